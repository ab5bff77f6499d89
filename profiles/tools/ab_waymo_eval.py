"""``WaymoDetectionEvaluator.update`` on the ``RangeDecoder.decode`` output of the bench model (rv-waymo, 4 sweeps of 64 x 2656), next to
the decode that produced it: the two calls interleaved round by round, each timed with HIP events, warm-up rounds discarded, the
shader clock sampled as ``bench.py`` does.  The random-init model puts almost nothing over ``min_confidence``, so a seeded 3 % of the
pixels are lifted over it (as profiles/tools/ab_nms_mode.py does).  Ground truth: about 100 boxes per sweep, every fifth detection of
the sweep moved by a few decimetres (so that gated pairs exist), interior points 1 .. 40.

    python profiles/tools/ab_waymo_eval.py [--rounds 40] [--warmup 5] > profiles/ab_waymo_eval.txt
"""
import argparse, json, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from bench import GpuSampler, build_model, synthetic_batch
from range_view_3d_detection_amd.evaluation import WaymoDetectionEvaluator
from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sweeps", type=int, default=4)
ap.add_argument("--gts-per-sweep", type=int, default=100)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_waymo_eval.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
torch.manual_seed(0)
NAMES = ["CYCLIST", "PEDESTRIAN", "VEHICLE"]
backbone, head = build_model("rv-waymo", len(NAMES))
backbone.to(dev).eval(); head.to(dev).eval()
batch = synthetic_batch(args.sweeps, 64, 2656, seed=1, device=dev, n_cls=len(NAMES))
with torch.no_grad():
    out, _ = head(backbone(batch), batch, return_loss=False)
    o = out[1][0]
    g = torch.Generator(device=dev).manual_seed(0)
    bump = (torch.rand(o["logits"].shape[0], 1, *o["logits"].shape[2:], device=dev, generator=g) < 0.03).float()
    o["logits"] = (o["logits"].float() + 3.0 * bump).contiguous()
    o["regressands"] = o["regressands"].float().contiguous()
dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
tasks = {0: NAMES}
post = {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "HARD"}
with torch.no_grad():
    params, scores, cats, bidx = dec.decode(out, post, tasks, use_nms=True)
# ground truth from the detections themselves (host side, once)
gh = torch.Generator().manual_seed(3)
p, b, c = params.cpu().double(), bidx.cpu().long(), cats.cpu().long()
rows = []
for s in range(args.sweeps):
    idx = torch.nonzero(b == s).flatten()
    idx = idx[torch.randperm(len(idx), generator=gh)[:args.gts_per_sweep]]
    box = p[idx].clone()
    box[:, :2] += torch.randn(len(idx), 2, generator=gh, dtype=torch.float64) * 0.2
    rows.append(torch.cat([box, torch.zeros(len(idx), 1, dtype=torch.float64), c[idx].double()[:, None], torch.full((len(idx), 1), float(s), dtype=torch.float64)], 1))
ann = torch.cat(rows).to(dev)
npts = torch.randint(1, 41, (ann.shape[0],), generator=gh).to(dev)
ev = WaymoDetectionEvaluator(idx_to_category=NAMES, max_sweeps=args.sweeps)
calls = {"decode": lambda: dec.decode(out, post, tasks, use_nms=True), "update": lambda: ev.update(params, scores, cats, bidx, ann, npts)}
ms = {k: [] for k in calls}
sampler = GpuSampler(0).start()
for r in range(args.warmup + args.rounds):
    for k in (list(calls) if r % 2 == 0 else list(calls)[::-1]):  # alternate which call goes first
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            calls[k]()
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            ms[k].append(e0.elapsed_time(e1))
cond = sampler.stop()
table = ev.compute()
per_class = [int(((cats == i)).sum()) for i in range(len(NAMES))]
rec = {"tool": "ab_waymo_eval", "model": "rv-waymo", "sweeps": args.sweeps, "H": 64, "W": 2656, "rounds": args.rounds, "warmup": args.warmup,
       "detections": int(params.shape[0]), "detections_per_class": per_class, "ground_truth": int(ann.shape[0]), "device": torch.cuda.get_device_name(0),
       "sclk_mhz_median": cond.get("sclk_mhz_median"), "power_w_median": cond.get("power_w_median"),
       "max_value": max(table.column("value").to_pylist())}
for k in calls:
    v = sorted(ms[k])
    rec[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(v[0], 4), "ms_p90": round(v[int(0.9 * (len(v) - 1))], 4)}
rec["update_ms_per_sweep_median"] = round(rec["update"]["ms_median"] / args.sweeps, 4)
print(json.dumps(rec))
