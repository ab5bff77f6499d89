"""AV2 ROI on the device against its NumPy restatement (tests/roi_ref.py), two pairs, interleaved round by round in one process:

  points   ``converters.av2.roi.roi_points`` on 4 sweeps of ~100k fp32 points from 2 logs (one launch, rows already on the device)
           against ``roi_ref.lookup_ref`` on the host copy of the same rows (what the reference's converter does through av2's map API,
           per sweep, on the host);
  update   ``DetectionEvaluator.update`` on one validation step (4 sweeps x 26 categories, ~2000 detections) without the filter, with
           ``roi=`` (two ``rv_roi_boxes`` launches + ``rv_eval_match_roi``), and the restatement of the filtered match on the host.

Device calls are timed with HIP events around the whole host call, host calls with ``time.perf_counter``; warm-up rounds are discarded, the
shader clock and the power are sampled as ``bench.py`` does.  The flags of both sides are compared once, before the timing.

    python profiles/tools/ab_roi.py [--rounds 30] [--warmup 5] [--points 100000] [--out profiles/ab_roi.txt]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import roi_ref as ref
from bench import GpuSampler
from range_view_3d_detection_amd.converters.av2.roi import RoiAtlas, roi_points
from range_view_3d_detection_amd.evaluation import DetectionCfg, DetectionEvaluator

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--points", type=int, default=100000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_roi.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_roi.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
g = np.random.default_rng(0)
B, N_CAT = 4, 26

# two logs: rasters of 0.3 m cells over 600 x 600 m, blobs of ROI; every sweep with its own pose near the raster's middle
layers = []
for k in range(2):
    coarse = g.random((50, 50)) < 0.6
    layers.append((np.kron(coarse, np.ones((40, 40), bool)).astype(np.uint8), (1 / 0.3, 300.0 + 7 * k, 300.0 - 5 * k)))
layer_index = np.array([0, 1, 0, 1])
poses = np.zeros((B, 3, 4))
for b in range(B):
    yaw = g.uniform(-np.pi, np.pi)
    poses[b, :, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
    poses[b, :, 3] = [g.uniform(-50, 50), g.uniform(-50, 50), 0.0]
atlas = RoiAtlas.from_rasters(["log0", "log1"], [l[0] for l in layers], [l[1] for l in layers]).to(dev)
to = lambda a, dtype=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)  # noqa: E731
d_layer, d_pose = to(layer_index.astype(np.int32)), to(poses)

# points: a lidar-like spread (most returns within 100 m, some to 250 m)
sizes = [args.points + 137 * b for b in range(B)]
xyz = np.concatenate([np.concatenate([g.normal(0, 45, (n, 2)), g.uniform(-2, 4, (n, 1))], 1) for n in sizes]).astype(np.float32)
sweep = np.repeat(np.arange(B), sizes)
offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
d_xyz, d_off, stray = to(xyz), to(offsets), torch.zeros((), dtype=torch.int64, device=dev)

# one validation step: boxes around ground truth, scores on a coarse grid
n_gt, n_dt = 300, 2000
gt_xy = g.uniform(-140, 140, (n_gt, 2))
yaw_q = lambda yaw: np.stack([np.cos(yaw / 2), np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2)], 1)  # noqa: E731
gts = np.concatenate([gt_xy, g.uniform(-1, 1, (n_gt, 1)), g.uniform(0.5, 6, (n_gt, 3)), yaw_q(g.uniform(-np.pi, np.pi, n_gt))], 1).astype(np.float32)
gt_sweep, gt_cat = g.integers(0, B, n_gt), g.integers(0, N_CAT, n_gt)
src = g.integers(0, n_gt, n_dt)
dts = gts[src].copy()
dts[:, :3] += g.normal(0, 1.0, (n_dt, 3)).astype(np.float32)
dt_sweep, dt_cat, scores = gt_sweep[src], gt_cat[src], np.round(g.random(n_dt), 2).astype(np.float32)
ann = np.zeros((n_gt, 13))
ann[:, :10], ann[:, 11], ann[:, 12] = gts, gt_cat, gt_sweep
names = [f"C{i}" for i in range(N_CAT)]
cfg_off, cfg_on = DetectionCfg(categories=tuple(names)), DetectionCfg(categories=tuple(names), eval_only_roi_instances=True)
ev_off, ev_on = DetectionEvaluator(cfg_off, names, max_sweeps=B), DetectionEvaluator(cfg_on, names, max_sweeps=B, atlas=atlas)
step = (to(dts), to(scores), to(dt_cat, torch.float32), to(dt_sweep, torch.float32), to(ann))
roi = (d_layer, d_pose)


def host_update():
    dt_roi, _ = ref.boxes_ref(dts, dt_sweep, layer_index, poses, layers)
    gt_roi, _ = ref.boxes_ref(gts, gt_sweep, layer_index, poses, layers)
    return ref.match_roi_ref(dts, scores, dt_sweep, dt_cat, dt_roi, gts, None, gt_roi, gt_sweep, gt_cat, B, N_CAT, cfg_on)


def reset_then(ev, **kw):
    ev._n = 0  # keep the accumulators' storage: the timed call does not grow them
    ev.update(*step, **kw)


device_calls = {"points_device": lambda: roi_points(d_xyz, d_off, d_layer, d_pose, atlas, stray=stray),
                "update_plain": lambda: reset_then(ev_off), "update_roi": lambda: reset_then(ev_on, roi=roi)}
host_calls = {"points_numpy": lambda: ref.lookup_ref(xyz, sweep, layer_index, poses, layers), "update_roi_numpy": host_update}

flags = device_calls["points_device"]().cpu().numpy()
want, _ = ref.lookup_ref(xyz, sweep, layer_index, poses, layers)
device_calls["update_plain"](), device_calls["update_roi"]()
torch.cuda.synchronize()
rec = {"tool": "ab_roi", "sweeps": B, "points": int(len(xyz)), "detections": n_dt, "ground_truth": n_gt, "categories": N_CAT, "rounds": args.rounds,
       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "points_equal_restatement": bool(np.array_equal(flags, want)),
       "points_within_roi": round(float(want.mean()), 4), "stray": int(stray)}
sampler = GpuSampler(0).start()
ms = {k: [] for k in list(device_calls) + list(host_calls)}
for r in range(args.warmup + args.rounds):
    order = list(ms) if r % 2 == 0 else list(ms)[::-1]  # alternate which call goes first
    for k in order:
        if k in device_calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_calls[k]()
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
        else:
            t0 = time.perf_counter()
            host_calls[k]()
            t = (time.perf_counter() - t0) * 1e3
        if r >= args.warmup:
            ms[k].append(t)
for k, v in ms.items():
    v = sorted(v)
    rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(v[0], 4), "ms_p90": round(v[int(0.9 * (len(v) - 1))], 4)}
rec["points_algorithmic_mb"] = round(len(xyz) * 14.0 / 1e6, 3)  # 12 B read, 1 B written, 1 raster byte per point
cond = sampler.stop()
rec["sclk_mhz_median"], rec["power_w_median"] = cond.get("sclk_mhz_median"), cond.get("power_w_median")
line = json.dumps(rec)
with open(args.out, "w") as fh:
    fh.write(line + "\n")
print(line)
