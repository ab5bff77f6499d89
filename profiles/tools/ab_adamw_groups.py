"""The optimiser step over rv-av2's parameter set (``bench.py``'s ``build_model``), clipping at 35 folded in, every variant on a copy of
its own of the parameters and moments and the same gradients:

  (a)  ``rv_adamw_step`` called directly on prebuilt tables (twice, as two variants: their difference is the run-to-run spread of this table);
  (b)  ``rv_adamw_step_groups`` called directly with one row;
  (a-step) ``optim.AdamW.step()`` with one group (= (a) plus the host side of a step: the gradient-pointer column and its upload);
  (c)  ``optim.AdamW.step()`` with the decay / no-decay split of ``configure_optimizers(no_weight_decay_1d=True)``;
  (d)  (c) with ``amsgrad=True``;
  (e)  ``clip_grad_norm_`` + ``torch.optim.AdamW`` (foreach) with the same two groups.

Variants are interleaved round by round (the order alternates), every step is timed with HIP events, warm-up rounds are discarded, the
shader clock and power are sampled as ``bench.py`` does.

    python profiles/tools/ab_adamw_groups.py [--rounds 60] [--warmup 10] > profiles/ab_adamw_groups.txt
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from bench import GpuSampler, build_model
from range_view_3d_detection_amd import _lib as L
from range_view_3d_detection_amd.nn.meta.arch import split_no_weight_decay_1d
from range_view_3d_detection_amd.optim import AdamW

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_adamw_groups.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
torch.manual_seed(0)
backbone, head = build_model("rv-av2", 26)
base = [p.detach().to(dev) for m in (backbone, head) for p in m.parameters()]
gen = torch.Generator(device=dev).manual_seed(0)
grads = [0.01 * torch.randn(p.shape, device=dev, generator=gen) for p in base]  # (norm far below 35: no variant changes them)
n_elems = sum(p.numel() for p in base)


def copy():
    ps = [torch.nn.Parameter(p.clone()) for p in base]
    for p, g in zip(ps, grads):
        p.grad = g
    return ps


def tables(ps):
    ce = int(L.load().rv_optim_chunk_elems())
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    tens = torch.tensor([[p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, m, v in zip(ps, ms, vs)], dtype=torch.int64).to(dev)
    chunks = [(i, c) for i, p in enumerate(ps) for c in range((p.numel() + ce - 1) // ce)]
    return {"keep": (ps, ms, vs), "tens": tens, "chunks": torch.tensor(chunks, dtype=torch.int32).to(dev), "n": len(chunks),
            "partial": torch.empty(len(chunks), device=dev), "row": torch.zeros(len(ps), dtype=torch.int32, device=dev), "norm": torch.zeros(1, device=dev)}


def direct(t):
    count = [0]

    def run():
        count[0] += 1
        L.call("rv_adamw_step", L.ptr(t["tens"]), L.ptr(t["chunks"]), t["n"], L.ptr(t["partial"]), 1e-3, 0.9, 0.999, 1e-8, 1e-2, count[0], 35.0,
               L.ptr(t["norm"]), L.stream_ptr())
    return run


def direct_groups(t):
    count = [0]

    def run():
        count[0] += 1
        rows = (L.AdamRow * 1)(L.AdamRow(1e-3, 0.9, 0.999, 1e-8, 1e-2, count[0], 0))
        L.call("rv_adamw_step_groups", L.ptr(t["tens"]), L.ptr(t["row"]), None, L.ptr(t["chunks"]), t["n"], L.ptr(t["partial"]), rows, 1, 35.0,
               L.ptr(t["norm"]), L.stream_ptr())
    return run


def torch_two_groups():
    ps = copy()
    for p in ps:
        p.grad = p.grad.clone()  # clip_grad_norm_ scales in place
    opt = torch.optim.AdamW(split_no_weight_decay_1d(ps, 1e-2), lr=1e-3)

    def run():
        torch.nn.utils.clip_grad_norm_(ps, 35.0)
        opt.step()
    return run


VARIANTS = {
    "(a) rv_adamw_step, direct (A)": direct(tables(copy())),
    "(a) rv_adamw_step, direct (B)": direct(tables(copy())),
    "(b) rv_adamw_step_groups, 1 row": direct_groups(tables(copy())),
    "(a-step) optim.AdamW, 1 group": AdamW(copy(), lr=1e-3, max_grad_norm=35.0).step,
    "(c) optim.AdamW, decay/no-decay": AdamW(split_no_weight_decay_1d(copy(), 1e-2), lr=1e-3, max_grad_norm=35.0).step,
    "(d) (c) with amsgrad": AdamW(split_no_weight_decay_1d(copy(), 1e-2), lr=1e-3, amsgrad=True, max_grad_norm=35.0).step,
    "(e) clip_grad_norm_ + torch AdamW": torch_two_groups(),
}
names = list(VARIANTS)
us = {n: [] for n in names}
sampler = GpuSampler(0).start()
for r in range(args.warmup + args.rounds):
    for n in (names if r % 2 == 0 else names[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        VARIANTS[n]()
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            us[n].append(1000.0 * e0.elapsed_time(e1))
cond = sampler.stop()
n_1d = sum(p.ndim <= 1 for p in base)
print(f"# ab_adamw_groups: one optimiser step over rv-av2's parameters ({len(base)} tensors, {n_1d} of them with ndim <= 1, {n_elems} elements), clipping at 35,")
print(f"# {args.rounds} rounds after {args.warmup} warm-up, interleaved, HIP events; microseconds per step")
print(f"# device {torch.cuda.get_device_name(0)}; sclk_mhz_median {cond.get('sclk_mhz_median')}, power_w_median {cond.get('power_w_median')}")
print(f"{'variant':36s} {'median':>8s} {'min':>8s} {'p10':>8s} {'p90':>8s} {'vs (A)':>7s}")
ref = statistics.median(us[names[0]])
for n in names:
    v = sorted(us[n])
    print(f"{n:36s} {statistics.median(v):8.1f} {v[0]:8.1f} {v[int(0.1 * (len(v) - 1))]:8.1f} {v[int(0.9 * (len(v) - 1))]:8.1f} {statistics.median(v) / ref:7.3f}")
