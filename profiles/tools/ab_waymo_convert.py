"""Waymo range images -> the detector's padded batch, three ways, for B frames of 64 x 2650 (synthetic frames of
tests/waymo_convert_ref.py, with pixel poses):

  (a) fused      ``converters.waymo.batch_from_range_images``: one launch (``rv_waymo_range_image_to_batch``);
  (b) unfused    ``range_image_to_sweep`` -> ``sweep_table`` -> ``range_view_from_table`` per frame, stacked: the route the package offers
                 without the fused entry (``range_view_from_table`` takes the table on the host, so the sweep crosses PCIe twice);
  (c) torch_fp64 the same declared arithmetic written with torch fp64 tensor ops on the device (what a user would otherwise write;
                 not the code under test).

The three are interleaved round by round in one process, each timed with HIP events, warm-up rounds discarded, the shader clock and the
power sampled as ``bench.py`` does.  ``achieved`` prices (a) at the algorithmic 77 B per pixel (40 read, 37 written) against 8 TB/s.
Condition on the fusion: (a) is not slower than (b) by more than the spread (p90 - min) of (b) in this same call.

    python profiles/tools/ab_waymo_convert.py [--rounds 30] [--warmup 5] [--batches 4 32] [--out profiles/ab_waymo_convert.txt]
"""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import waymo_convert_ref as ref
from bench import GpuSampler
from range_view_3d_detection_amd.converters.waymo import batch_from_range_images, range_image_to_sweep, sweep_table
from range_view_3d_detection_amd.prototype.loader import range_view_from_table

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="+", default=[4, 32])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_waymo_convert.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_waymo_convert.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
H, W, PAD = 64, 2650, 3
NAMES = list(ref.WAYMO_FEATURES)
CFG = {"feature_column_names": NAMES, "height": H, "width": W}


def torch_fp64(ri, ext, incl, pp, inv):
    """The declared arithmetic with torch tensor ops (fp64 on the device), constant padding."""
    B = ri.shape[0]
    valid = (ri[..., 0] > 0) & (ri[..., 3] != 1.0)
    c = torch.arange(W, dtype=torch.float64, device=dev)
    az = ((2.0 * ((W - c - 0.5) / W) - 1.0) * math.pi)[None, None, :] - torch.atan2(ext[:, 1, 0], ext[:, 0, 0])[:, None, None]
    rng = ri[..., 0].double()
    ci, si = torch.cos(incl)[:, :, None], torch.sin(incl)[:, :, None]
    p = torch.stack([rng * (torch.cos(az) * ci), rng * (torch.sin(az) * ci), rng * si], -1)
    p = torch.einsum("bij,bhwj->bhwi", ext[:, :3, :3], p) + ext[:, None, None, :3, 3]
    q = pp.double()
    sr, cr, sp, cp, sy, cy = torch.sin(q[..., 0]), torch.cos(q[..., 0]), torch.sin(q[..., 1]), torch.cos(q[..., 1]), torch.sin(q[..., 2]), torch.cos(q[..., 2])
    R = torch.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, -sp, cp * sr, cp * cr], -1)
    world = torch.einsum("bhwij,bhwj->bhwi", R.view(B, H, W, 3, 3), p) + q[..., 3:]
    p = torch.einsum("bij,bhwj->bhwi", inv[:, :, :3], world) + inv[:, None, None, :, 3]
    sweep = torch.where(valid[..., None], torch.cat([ri[..., :3], p.float()], -1), torch.zeros((), device=dev))
    chan = {n: sweep[..., i] for i, n in enumerate(ref.SWEEP_CHANNELS)}
    chan["intensity"] = torch.tanh(chan["intensity"])
    padw = lambda t: torch.nn.functional.pad(t, (PAD, PAD))  # noqa: E731
    return {"features": padw(torch.stack([chan[n] for n in NAMES], 1)), "cart": padw(torch.stack([chan[n] for n in ("x", "y", "z")], 1)),
            "mask": padw(valid[:, None]), "num_pts": valid.flatten(1).sum(1)}


def unfused(dev_args):
    sweep, _ = range_image_to_sweep(*dev_args)
    items = [range_view_from_table(sweep_table(sweep[b]), CFG, "waymo", device=dev) for b in range(sweep.shape[0])]
    return {k: torch.stack([it[k] for it in items]) for k in ("features", "cart", "mask")}


rec = {"tool": "ab_waymo_convert", "H": H, "W": W, "padded_W": W + 2 * PAD, "rounds": args.rounds, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
       "bytes_per_pixel": 77, "hbm_roofline_tb_s": 8.0, "sizes": {}}
sampler = GpuSampler(0).start()
for B in args.batches:
    f = ref.make_frames(1, B, H, W, offset=1e3)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    dev_args = (to(f["range_image"]), to(f["extrinsic"]), to(f["inclination"]), to(f["pixel_pose"]), to(f["frame_pose"]))
    inv = torch.linalg.inv(dev_args[4])[:, :3, :].contiguous()
    calls = {"fused": lambda: batch_from_range_images(*dev_args, CFG), "unfused": lambda: unfused(dev_args),
             "torch_fp64": lambda: torch_fp64(dev_args[0], dev_args[1], dev_args[2], dev_args[3], inv)}
    a, b, c = calls["fused"](), calls["unfused"](), calls["torch_fp64"]()
    agree = all(torch.equal(a[k], b[k]) for k in ("features", "cart", "mask"))
    torch_max_diff = float((a["cart"].double() - c["cart"].double()).abs().max())
    del a, b, c
    ms = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for k in (list(calls) if r % 2 == 0 else list(calls)[::-1]):  # alternate which call goes first
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls[k]()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    size = {"frames": B, "fused_equals_unfused": agree, "torch_fp64_max_abs_diff_m": torch_max_diff}
    for k in calls:
        v = sorted(ms[k])
        size[k] = {"ms_median": round(statistics.median(v), 4), "ms_min": round(v[0], 4), "ms_p90": round(v[int(0.9 * (len(v) - 1))], 4)}
    nbytes = 77.0 * B * H * W
    size["algorithmic_mb"] = round(nbytes / 1e6, 2)
    size["fused_achieved_tb_s"] = round(nbytes / (size["fused"]["ms_median"] * 1e-3) / 1e12, 4)
    size["fused_fraction_of_roofline"] = round(size["fused_achieved_tb_s"] / 8.0, 4)
    spread = size["unfused"]["ms_p90"] - size["unfused"]["ms_min"]
    size["unfused_spread_ms"] = round(spread, 4)
    size["fusion_earns_its_entry"] = bool(size["fused"]["ms_median"] <= size["unfused"]["ms_median"] + spread)
    rec["sizes"][str(B)] = size
cond = sampler.stop()
rec["sclk_mhz_median"], rec["power_w_median"] = cond.get("sclk_mhz_median"), cond.get("power_w_median")
line = json.dumps(rec)
with open(args.out, "w") as fh:
    fh.write(line + "\n")
print(line)
