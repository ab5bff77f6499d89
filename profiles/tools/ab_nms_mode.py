"""``RangeDecoder.decode`` with ``nms_mode`` WEIGHTED against HARD on the SAME eval-forward output of the bench model (rv-av2, 4 sweeps of
64 x 2048): the two variants interleaved round by round, every call timed with HIP events, warm-up rounds discarded, the shader clock
sampled as ``bench.py`` does.  The random-init model puts almost nothing over ``min_confidence``, so a seeded 3 % of the pixels are lifted
over it (as profiles/tools/infer_time.py does): a few thousand candidates per sweep, neighbouring pixels decoding to overlapping boxes.

    python profiles/tools/ab_nms_mode.py [--rounds 40] [--warmup 5] > profiles/ab_nms_mode.txt
"""
import argparse, json, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from bench import GpuSampler, build_model, synthetic_batch
from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sweeps", type=int, default=4)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_nms_mode.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
torch.manual_seed(0)
N_CLS = 26
backbone, head = build_model("rv-av2", N_CLS)
backbone.to(dev).eval(); head.to(dev).eval()
batch = synthetic_batch(args.sweeps, 64, 2048, seed=1, device=dev)
with torch.no_grad():
    out, _ = head(backbone(batch), batch, return_loss=False)
    o = out[1][0]
    g = torch.Generator(device=dev).manual_seed(0)
    bump = (torch.rand(o["logits"].shape[0], 1, *o["logits"].shape[2:], device=dev, generator=g) < 0.03).float()
    o["logits"] = (o["logits"].float() + 3.0 * bump).contiguous()
    o["regressands"] = o["regressands"].float().contiguous()
dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
tasks = {0: [f"C{i}" for i in range(N_CLS)]}
post = {m: {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": m} for m in ("WEIGHTED", "HARD")}
modes = ("WEIGHTED", "HARD")
ms = {m: [] for m in modes}
rows = {}
sampler = GpuSampler(0).start()
for r in range(args.warmup + args.rounds):
    for m in (modes if r % 2 == 0 else modes[::-1]):  # alternate which variant goes first
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            res = dec.decode(out, post[m], tasks, use_nms=True)
        e1.record()
        e1.synchronize()
        rows[m] = int(res[0].shape[0])
        if r >= args.warmup:
            ms[m].append(e0.elapsed_time(e1))
cond = sampler.stop()
n_cand = int((torch.sigmoid(o["logits"]).amax(1) * batch["mask"][:, 0] >= 0.1).sum())
rec = {"tool": "ab_nms_mode", "model": "rv-av2", "sweeps": args.sweeps, "H": 64, "W": 2048, "n_classes": N_CLS, "rounds": args.rounds, "warmup": args.warmup,
       "pixels_over_min_confidence_before_band_sampling": n_cand, "device": torch.cuda.get_device_name(0),
       "sclk_mhz_median": cond.get("sclk_mhz_median"), "power_w_median": cond.get("power_w_median")}
for m in modes:
    v = sorted(ms[m])
    rec[m] = {"decode_ms_median": round(statistics.median(v), 4), "decode_ms_min": round(v[0], 4), "decode_ms_p90": round(v[int(0.9 * (len(v) - 1))], 4),
              "rows_out": rows[m]}
rec["hard_over_weighted_median"] = round(rec["HARD"]["decode_ms_median"] / rec["WEIGHTED"]["decode_ms_median"], 4)
print(json.dumps(rec))
