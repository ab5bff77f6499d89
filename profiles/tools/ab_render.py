"""``rendering.tensorboard.draw_detections`` on one rv-av2-shaped eval output (one sample of 64 x 1808, one task, 100 detections, 30
annotations, the default 1000 x 1000 bird's-eye view) against the host route: the inputs copied to the host as the reference copies
them, then the NumPy restatement ``tests/render_ref.py`` (its 3-D IoU on the device, the reference's one GPU step).  The two
interleaved round by round, warm-up rounds discarded; the device route timed with HIP events (the launches) and on the host (launches +
the upload of the box rows), the host route on the host, the shader clock sampled as ``bench.py`` does.  ``to_host_ms`` is the single
device-to-host copy ``to_logger`` adds.  Library entries per image are counted on one extra call.  A record, not a gate: the
restatement is written to be read, not to be fast.

    python profiles/tools/ab_render.py [--rounds 20] [--warmup 3] > profiles/ab_render.txt
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import render_ref as R
from waymo_eval_ref import boxes_from_rows
from bench import GpuSampler, synthetic_batch
from range_view_3d_detection_amd import _lib as L
from range_view_3d_detection_amd.rendering import tensorboard as tb

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_render.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
H, W, N_CLS, N_DT, N_GT = 64, 1808, 5, 100, 30
MAX_SIDE, MPP = 75.0, 0.15
sb = synthetic_batch(1, H, W, seed=1, device="cpu", boxes_per_sweep=N_GT, n_cls=N_CLS)
g = torch.Generator().manual_seed(2)
ann = sb["annotations"].double()[:N_GT]
ann[:, 12] = 0
rows = torch.cat([ann[:, :10], ann[torch.randint(0, len(ann), (N_DT - len(ann),), generator=g), :10]])
rows[:, :2] += torch.randn(N_DT, 2, generator=g, dtype=torch.float64) * 0.4
scores = torch.rand(N_DT, generator=g)
dts = {**{c: rows[:, j].float().numpy() for j, c in enumerate(tb.COLS)}, "score": scores.numpy(), "batch_index": np.zeros(N_DT, np.int32)}
outputs = {"head": {1: {"cart": sb["cart"].to(dev), "mask": sb["mask"].to(dev),
                        0: {"logits": (torch.randn(1, N_CLS, H, W, generator=g) * 3 - 3).to(dev)}}}}
data = {"annotations": ann}
tables = {k: getattr(tb, k).numpy() for k in ("TURBO_R", "VIRIDIS")}


def device_route():
    return tb.draw_detections(dts, None, data, outputs, max_num_dts=N_DT, max_side=MAX_SIDE, meter_per_px=MPP)


def host_route():
    level = outputs["head"][1]
    cart, mask, logits = level["cart"][0].cpu().numpy(), level["mask"][0, 0].cpu().numpy(), level[0]["logits"][0].cpu().numpy()
    lik = R.normalize_apply_colormap(R.plane_likelihood(logits), tables["VIRIDIS"], mask)
    rng = R.normalize_apply_colormap(R.plane_norm(cart), tables["TURBO_R"], mask)
    bev = R.bev_points(cart, MAX_SIDE, MPP)
    order = np.argsort(-dts["score"], kind="stable")
    gts, det = boxes_from_rows(ann[:, :10].numpy()), boxes_from_rows(rows.numpy()[order])
    iou = tb.boxes_iou3d(torch.from_numpy(det).to(dev), torch.from_numpy(gts).to(dev)).cpu().numpy()
    boxes = np.concatenate([gts, det])
    sc = np.concatenate([np.ones(len(gts), np.float32), dts["score"][order]])
    chans = np.concatenate([np.full(len(gts), R.BLUE, np.uint8), R.detection_channels(iou.max(1))])
    return R.stack([lik, rng, lik], ["likelihood", "range", "likelihood"], R.draw_boxes(bev, boxes, sc, chans, MAX_SIDE, MPP))


calls = []
inner = L._call
L._call = lambda name, *a: (calls.append(name), inner(name, *a))[1]
image = device_route()
L._call = inner
differing = int((image.cpu().numpy() != host_route()).any(0).sum())  # (the likelihood plane's last bits are each library's expf)
ms = {"device_events": [], "device_host": [], "host_route": [], "to_host": []}
sampler = GpuSampler(0).start()
for rnd in range(args.warmup + args.rounds):
    for which in (("device", "host") if rnd % 2 == 0 else ("host", "device")):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "device":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            image = device_route()
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            image.cpu()
            t2 = time.perf_counter()
            if rnd >= args.warmup:
                ms["device_events"].append(e0.elapsed_time(e1)), ms["device_host"].append(1e3 * (t1 - t0)), ms["to_host"].append(1e3 * (t2 - t1))
        else:
            host_route()
            if rnd >= args.warmup:
                ms["host_route"].append(1e3 * (time.perf_counter() - t0))
cond = sampler.stop()
rec = {"tool": "ab_render", "H": H, "W": W, "classes": N_CLS, "detections": N_DT, "annotations": N_GT, "bev_side": R.bev_side(MAX_SIDE, MPP),
       "image": list(image.shape), "panels": 3, "rounds": args.rounds, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
       "sclk_mhz_median": cond.get("sclk_mhz_median"), "power_w_median": cond.get("power_w_median"),
       "library_entries_per_image": len(calls), "library_entries": calls, "pixels_differing_between_the_routes": differing}
for k, v in ms.items():
    v = sorted(v)
    rec[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "p90": round(v[int(0.9 * (len(v) - 1))], 4)}
print(json.dumps(rec))
