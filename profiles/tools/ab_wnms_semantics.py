"""Cost of carrying the weighted-NMS choices per call: ``RangeDecoder.decode`` WEIGHTED on the input of profiles/tools/ab_nms_mode.py
(rv-av2 eval forward, 4 sweeps of 64 x 2048, a seeded 3 % of the pixels lifted over ``min_confidence``), the PARENT commit's library against
this tree's, in ONE process: both libraries are loaded (each typed from its own header) and the binding's handle is switched between
calls, so the variants are interleaved call by call under the same clocks.  Per round, in rotating order:

    parent_a, parent_b   the parent library, twice -- two interleaved series of the SAME code: the difference of their medians is the
                         spread that the run itself shows between two runs of the parent library;
    head_flags0          this tree's library, no ``wnms_semantics`` (flags = 0);
    head_<option>        this tree's library with one option set (the four single-flag settings).

Every call is timed with HIP events; warm-up rounds are discarded; the shader clock is sampled as bench.py does.  Bar: the median of
head_flags0 may exceed the parent's median (all parent samples) by no more than the parent_a / parent_b spread.

    python profiles/tools/ab_wnms_semantics.py --parent-lib P/librv3d_hip.so --parent-header P/rv3d.h [--rounds 60] [--warmup 8]
"""
import argparse, json, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from bench import GpuSampler, build_model, synthetic_batch
from range_view_3d_detection_amd import _lib as L
from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--parent-header", required=True)
ap.add_argument("--rounds", type=int, default=60)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--sweeps", type=int, default=4)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_wnms_semantics.py needs an MI355X: there is nothing to time without one")
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
torch.cuda.synchronize()

head_lib = L.load()
L.HEADER_PATH, keep_header = args.parent_header, L.HEADER_PATH  # the parent library exports what the PARENT header declares
L.prototypes.cache_clear(); L.included_prototypes.cache_clear()
parent_lib = L._dlopen(args.parent_lib)
L.HEADER_PATH = keep_header
L.prototypes.cache_clear(); L.included_prototypes.cache_clear()

dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
tasks = {0: [f"C{i}" for i in range(N_CLS)]}
base = {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "WEIGHTED"}
options = {"merge_set_ALL": {"merge_set": "ALL"}, "score_KEEPER": {"score": "KEEPER"}, "nms_compare_GE": {"nms_compare": "GE"},
           "merge_compare_GE": {"merge_compare": "GE"}}
variants = {"parent_a": (parent_lib, base), "parent_b": (parent_lib, base), "head_flags0": (head_lib, base)}
variants.update({f"head_{k}": (head_lib, {**base, "wnms_semantics": v}) for k, v in options.items()})
names = list(variants)
ms = {v: [] for v in names}
rows, first = {}, {}
sampler = GpuSampler(0).start()
for r in range(args.warmup + args.rounds):
    k = r % len(names)
    for v in names[k:] + names[:k]:  # rotate which variant goes first
        L._lib, post = variants[v]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            res = dec.decode(out, post, tasks, use_nms=True)
        e1.record()
        e1.synchronize()
        rows[v] = int(res[0].shape[0])
        first.setdefault(v, res)
        if r >= args.warmup:
            ms[v].append(e0.elapsed_time(e1))
L._lib = head_lib
cond = sampler.stop()
same = all(torch.equal(a, b) for a, b in zip(first["parent_a"], first["head_flags0"]))
rec = {"tool": "ab_wnms_semantics", "model": "rv-av2", "sweeps": args.sweeps, "H": 64, "W": 2048, "n_classes": N_CLS, "rounds": args.rounds,
       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sclk_mhz_median": cond.get("sclk_mhz_median"),
       "power_w_median": cond.get("power_w_median"), "head_flags0_rows_bit_equal_to_parent": same}
for v in names:
    s = sorted(ms[v])
    rec[v] = {"decode_ms_median": round(statistics.median(s), 4), "decode_ms_min": round(s[0], 4), "decode_ms_p90": round(s[int(0.9 * (len(s) - 1))], 4),
              "rows_out": rows[v]}
parent_median = statistics.median(ms["parent_a"] + ms["parent_b"])
spread = abs(rec["parent_a"]["decode_ms_median"] - rec["parent_b"]["decode_ms_median"])
rec["parent_median_ms"] = round(parent_median, 4)
rec["parent_a_b_spread_ms"] = round(spread, 4)
rec["head_flags0_minus_parent_ms"] = round(rec["head_flags0"]["decode_ms_median"] - parent_median, 4)
rec["within_bar"] = rec["head_flags0"]["decode_ms_median"] <= parent_median + spread
print(json.dumps(rec))
