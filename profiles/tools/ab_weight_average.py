"""One optimiser step + one update of an averaged model (EMA, decay 0.999) over rv-av2's parameters and buffers (``bench.py``'s
``build_model``), clipping at 35 folded in, every variant on a copy of its own of the model and the same gradients:

  (0)  ``optim.AdamW.step()`` alone (what the update is added to);
  (a)  ``optim.AveragedModel`` fused into the step (``rv_adamw_step_groups_avg``) + ``update_parameters`` (``rv_average_tensors`` for the rest);
  (s)  ``optim.AdamW.step()`` + ``optim.AveragedModel.update_parameters`` unfused (``rv_average_tensors`` for everything);
  (b)  ``optim.AdamW.step()`` + ``torch.optim.swa_utils.AveragedModel.update_parameters`` (``get_ema_multi_avg_fn``: foreach lerp, one
       ``copy_`` per buffer under ``use_buffers=False``);

(a), (s) and (b) with ``use_buffers`` False and True.  Variants are interleaved round by round (the order alternates), every step is timed
with HIP events, warm-up rounds are discarded, the shader clock and power are sampled as ``bench.py`` does.  Launch counts of one
steady-state step: library calls from the binding's call log, device kernels and memory copies from ``torch.profiler``.
The model is stepped in isolation, so a step here is bound by its HOST side (walking the module tree for parameters and buffers costs
about a millisecond per walk, in torch's class as in ours); in a training loop whose host runs ahead of the device that work overlaps
kernels still in flight.  ``busy``: the sum of the device events' durations of a profiled step -- what the device itself spends --, median
of five profiled steps.

    python profiles/tools/ab_weight_average.py [--rounds 40] [--warmup 8] > profiles/ab_weight_average.txt
"""
import argparse, copy, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from torch.optim.swa_utils import get_ema_multi_avg_fn
from bench import GpuSampler, build_model
from range_view_3d_detection_amd import _lib as L
from range_view_3d_detection_amd.optim import AdamW, AveragedModel

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ab_weight_average.py needs an MI355X: there is nothing to time without one")
dev = torch.device("cuda:0")
torch.manual_seed(0)
base = torch.nn.ModuleList(build_model("rv-av2", 26)).to(dev)
gen = torch.Generator(device=dev).manual_seed(0)
grads = [0.01 * torch.randn(p.shape, device=dev, generator=gen) for p in base.parameters()]  # (norm far below 35: no variant changes them)
n_elems = sum(p.numel() for p in base.parameters())
n_buffers = sum(1 for _ in base.buffers())
DECAY = 0.999


def model_and_optimiser():
    model = copy.deepcopy(base)
    for p, g in zip(model.parameters(), grads):
        p.grad = g
    return model, AdamW(list(model.parameters()), lr=1e-3, max_grad_norm=35.0)


def step_alone():
    _, opt = model_and_optimiser()
    return opt.step


def ours(use_buffers, fused):
    model, opt = model_and_optimiser()
    ema = AveragedModel(model, use_buffers=use_buffers, decay=DECAY)
    if fused:
        ema.fuse(opt, model)

    def run():
        opt.step()
        ema.update_parameters(model)
    return run


def torchs(use_buffers):
    model, opt = model_and_optimiser()
    ema = torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(DECAY), use_buffers=use_buffers)

    def run():
        opt.step()
        ema.update_parameters(model)
    return run


VARIANTS = {"(0) optim.AdamW.step() alone": step_alone()}
for ub in (False, True):
    VARIANTS[f"(a) fused step + update, use_buffers={ub}"] = ours(ub, True)
    VARIANTS[f"(s) step + our update, use_buffers={ub}"] = ours(ub, False)
    VARIANTS[f"(b) step + torch's update, use_buffers={ub}"] = torchs(ub)
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

# launch counts and device time of five more (steady-state) steps of every variant, each under the profiler
counts = {}
real = L._call
for n in names:
    busy = []
    for _ in range(5):
        calls = []

        def spy(name, *a):
            calls.append(name)
            return real(name, *a)

        L._call = spy
        try:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
                VARIANTS[n]()
                torch.cuda.synchronize()
        finally:
            L._call = real
        device = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
        copies = sum(1 for ev in device if "memcpy" in ev.name.lower() or "memset" in ev.name.lower())
        busy.append(sum(ev.time_range.elapsed_us() for ev in device))
    counts[n] = (len(calls), len(device) - copies, copies, statistics.median(busy))

print(f"# ab_weight_average: one optimiser step + one EMA update (decay {DECAY}) over rv-av2 ({len(grads)} parameter tensors, {n_elems} elements, "
      f"{n_buffers} buffers), clipping at 35,")
print(f"# {args.rounds} rounds after {args.warmup} warm-up, interleaved, HIP events; microseconds per step; launches of one steady-state step")
print(f"# device {torch.cuda.get_device_name(0)}; sclk_mhz_median {cond.get('sclk_mhz_median')}, power_w_median {cond.get('power_w_median')}")
print(f"{'variant':46s} {'median':>8s} {'min':>8s} {'p10':>8s} {'p90':>8s} {'- (0)':>8s} {'lib calls':>9s} {'kernels':>8s} {'memcpys':>8s} {'busy':>8s}")
ref = statistics.median(us[names[0]])
for n in names:
    v = sorted(us[n])
    print(f"{n:46s} {statistics.median(v):8.1f} {v[0]:8.1f} {v[int(0.1 * (len(v) - 1))]:8.1f} {v[int(0.9 * (len(v) - 1))]:8.1f} "
          f"{statistics.median(v) - ref:8.1f} {counts[n][0]:9d} {counts[n][1]:8d} {counts[n][2]:8d} {counts[n][3]:8.1f}")
