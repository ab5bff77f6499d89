"""``train_batch_from_tables`` with and without the object database (``db`` / ``db_config``) on rv-av2's loader shape: 4 sweeps of
64 x 1800 x 5 features, 15 objects drawn per sweep from a synthetic database of 600 objects.  The two variants interleaved round by round,
every call timed on the host from before the call to after a device synchronisation (the chain uploads the tables, so it holds host work),
warm-up rounds discarded, the shader clock sampled as ``bench.py`` does.  ``paste_ms``: ``paste_database`` alone on the unpadded batch,
timed with HIP events (the launches) and on the host (launches + the one B x S-byte copy + the annotation merge).

    python profiles/tools/ab_db_paste.py [--rounds 40] [--warmup 5] > profiles/ab_db_paste.txt
"""
import argparse, json, os, random, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from bench import GpuSampler, synthetic_batch
from range_view_3d_detection_amd.prototype import loader as ld
from range_view_3d_detection_amd.prototype.database import ObjectDatabase, draw_database_samples, paste_database

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sweeps", type=int, default=4)
ap.add_argument("--objects", type=int, default=15)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_db_paste.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
B, H, W = args.sweeps, 64, 1800
NAMES = ["intensity", "range", "x", "y", "z"]
CATS = ["REGULAR_VEHICLE", "PEDESTRIAN", "BUS"]
cfg = {"feature_column_names": NAMES, "filter_roi": False, "height": H, "width": W}
tasks = {0: CATS}
sb = synthetic_batch(B, H, W, seed=1, device="cpu", boxes_per_sweep=16, n_cls=3)
tables = []
for b in range(B):
    cart = sb["cart"][b].numpy().reshape(3, -1)
    valid = sb["mask"][b].numpy().reshape(-1)
    tables.append({"x": cart[0] * valid, "y": cart[1] * valid, "z": cart[2] * valid, "range": (np.linalg.norm(cart, axis=0) * valid).astype(np.float32),
                   "intensity": (np.arange(H * W) % 251).astype(np.float32) * valid})
ann = sb["annotations"].double()
# a synthetic database: objects of 1 .. ~700 points in blocks of pixels, boxes scattered in BEV
rng = np.random.default_rng(0)
pts, rngs, idx, offsets, boxes, cats = [], [], [], [0], [], []
for i in range(600):
    hh, ww = int(rng.integers(1, 12)), int(rng.integers(1, 60))
    r0, c0 = int(rng.integers(0, H - hh + 1)), int(rng.integers(0, W - ww + 1))
    rr, cc = np.meshgrid(np.arange(r0, r0 + hh), np.arange(c0, c0 + ww), indexing="ij")
    px = (rr.reshape(-1) * W + cc.reshape(-1))
    n = px.size
    r = (rng.uniform(5, 60) + rng.random(n) * 4.0).astype(np.float32)
    xyz = (rng.normal(size=(n, 3)) * 20).astype(np.float32)
    pts.append(np.concatenate([xyz, rng.random((n, 1)).astype(np.float32) * 255, r[:, None], xyz], axis=1))
    rngs.append(r), idx.append(px), offsets.append(offsets[-1] + n)
    yaw = rng.uniform(-np.pi, np.pi)
    boxes.append([rng.uniform(-100, 100), rng.uniform(-100, 100), 0.0, rng.uniform(0.5, 10), rng.uniform(0.5, 3), 1.5, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
    cats.append(CATS[i % 3])
db = ObjectDatabase(np.asarray(boxes), cats, list(range(600)), np.concatenate(pts), np.concatenate(rngs), np.concatenate(idx), np.asarray(offsets), NAMES, H, W).to(dev)
db_config = {c: args.objects // 3 for c in CATS}
aug = {"flip_azimuth": {"p": 0.5}, "random_rotation": {"low": -0.78539816, "high": 0.78539816, "p": 1.0}, "random_global_scale": {"low": 0.95, "high": 1.05}}
variants = {"without_db": {}, "with_db": {"db": db, "db_config": db_config, "tasks": tasks}}
order = tuple(variants)
ms = {k: [] for k in order}
paste_dev, paste_host, pasted = [], [], []
r = random.Random(0)
sampler = GpuSampler(0).start()
for rnd in range(args.warmup + args.rounds):
    for k in (order if rnd % 2 == 0 else order[::-1]):  # alternate which variant goes first
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ld.train_batch_from_tables(tables, ann, cfg, "av2", aug, 1, "constant", rng=r, device=dev, **variants[k])
        torch.cuda.synchronize()
        if rnd >= args.warmup:
            ms[k].append(1e3 * (time.perf_counter() - t0))
    # the paste alone, on an unpadded batch that already sits on the device
    items = [ld.range_view_from_table(t, cfg, "av2", device=dev, pad=False) for t in tables]
    batch = {k: torch.stack([it[k] for it in items]) for k in ("features", "mask", "cart")}
    batch["annotations"] = ann
    draws = [draw_database_samples(db, db_config, r) for _ in range(B)]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    res = paste_database(batch, db, draws, tasks)
    e1.record()
    e1.synchronize()
    if rnd >= args.warmup:
        paste_host.append(1e3 * (time.perf_counter() - t0))
        paste_dev.append(e0.elapsed_time(e1))
        pasted.append(sum(len(p) for p in res["pasted"]))
cond = sampler.stop()
med = lambda v: round(statistics.median(v), 4)  # noqa: E731
rec = {"tool": "ab_db_paste", "sweeps": B, "H": H, "W": W, "features": len(NAMES), "objects_drawn_per_sweep": sum(db_config.values()),
       "objects_pasted_per_batch_median": statistics.median(pasted), "database_objects": len(db), "database_points": int(db.offsets[-1]),
       "rounds": args.rounds, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sclk_mhz_median": cond.get("sclk_mhz_median"),
       "power_w_median": cond.get("power_w_median")}
for k in order:
    v = sorted(ms[k])
    rec[k] = {"chain_ms_median": med(v), "chain_ms_min": round(v[0], 4), "chain_ms_p90": round(v[int(0.9 * (len(v) - 1))], 4)}
rec["with_minus_without_ms_median"] = round(rec["with_db"]["chain_ms_median"] - rec["without_db"]["chain_ms_median"], 4)
rec["paste_ms"] = {"device_events_median": med(paste_dev), "device_events_min": round(min(paste_dev), 4), "host_median": med(paste_host),
                   "host_min": round(min(paste_host), 4)}
print(json.dumps(rec))
