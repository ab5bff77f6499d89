"""Two real ranks with DIFFERENT data, on one GPU: the launcher, the shared test cases and the yardstick arithmetic of
tests/test_gpu_two_rank.py, tests/test_two_rank_cpu.py, tests/two_rank_worker.py and ``tests/tools/emulation_yardstick.py two-rank``.
A plain helper module (no fixtures, nothing pytest collects).

Launcher (``launch``): ``world`` fresh child processes of tests/two_rank_worker.py (``subprocess.Popen([sys.executable, ...])``; the
parent needs no GPU context), rendezvous through a ``file://`` store inside ``tmp_path`` (no fixed port), gloo, both ranks on
``cuda:0``; each rank writes ``tmp_path/rank{r}.pt``.  The parent polls with a time limit; on the first non-zero exit or on the limit it
kills what is left and fails with the tail of the output.  No retries, at most ``world`` <= 2 children at any time.

Cases (``build_case``): the batch of four (c32) / two (rv-av2 widths) sweeps whose LAST sweeps -- rank 1's share -- are made
heterogeneous (features scaled and offset per channel, coordinate axes permuted and stretched), so that rank-local and global BatchNorm
statistics differ by O(1); the fixed
linear functional of the head outputs (``functional``) whose per-rank gradients add up to the gradient of one model on all sweeps.
"""

from __future__ import annotations

import os
import subprocess
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "two_rank_worker.py")
YARDSTICK = os.path.join(HERE, "golden", "two_rank_yardstick.json")


class TwoRankFailure(AssertionError):
    """A rank exited non-zero, or the launch ran into its time limit."""


def _tail(path: str, n: int = 3000) -> str:
    try:
        with open(path, "r", errors="replace") as f:
            return f.read()[-n:]
    except OSError:
        return "<no output>"


def launch(mode: str, world: int, tmp_path, args: Sequence[str] = (), limit_s: float = 120.0, collective_timeout_s: Optional[float] = None) -> List[dict]:
    """Run ``world`` (1 or 2) ranks of the worker in ``mode``; returns what each wrote to ``rank{r}.pt``, in rank order.  The collective
    timeout inside the workers (``init_process_group(timeout=...)``) is shorter than ``limit_s``: a rank whose peer died leaves its
    collective by itself even if the parent were gone."""
    import torch

    assert world in (1, 2), world
    tmp_path = str(tmp_path)
    for stale in ["rendezvous"] + [f"rank{r}.pt" for r in range(world)]:
        if os.path.exists(os.path.join(tmp_path, stale)):
            os.remove(os.path.join(tmp_path, stale))
    if collective_timeout_s is None:
        collective_timeout_s = min(60.0, 0.5 * limit_s)
    assert collective_timeout_s < limit_s
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONUNBUFFERED="1")
    procs, logs = [], []
    t0 = time.monotonic()
    try:
        for r in range(world):
            log = os.path.join(tmp_path, f"rank{r}.log")
            logs.append(log)
            with open(log, "w") as out:
                procs.append(subprocess.Popen([sys.executable, WORKER, "--mode", mode, "--rank", str(r), "--world", str(world), "--dir", tmp_path,
                                               "--collective-timeout", str(collective_timeout_s), *[str(a) for a in args]],
                                              env=env, cwd=ROOT, stdout=out, stderr=subprocess.STDOUT))
        live = set(range(world))
        while live:
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0:
                    raise TwoRankFailure(f"rank {r} of {world} (mode {mode}) exited with {code} after {time.monotonic() - t0:.1f} s; nothing else is started.\n"
                                         + "".join(f"--- rank {q} ---\n{_tail(logs[q])}\n" for q in range(world)))
            if live and time.monotonic() - t0 > limit_s:
                raise TwoRankFailure(f"ranks {sorted(live)} of {world} (mode {mode}) still running after the limit of {limit_s:.0f} s; killed.\n"
                                     + "".join(f"--- rank {q} ---\n{_tail(logs[q])}\n" for q in range(world)))
            if live:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    seconds = time.monotonic() - t0
    print(f"[two_rank] mode {mode} {' '.join(str(a) for a in args)}: {world} rank(s) in {seconds:.1f} s (limit {limit_s:.0f} s)")
    launch.last_seconds = seconds
    return [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(world)]


launch.last_seconds = 0.0

# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
# name -> (widths, classes, sweeps, H, W, sweeps per rank, BatchNorm bias shifts)
CASES = {"c32": ("c32", 5, 4, 16, 256, (3, 1), (6.0, 3.0)),
         "rv-av2": ("rv-av2", 26, 2, 64, 256, (1, 1), (3.0,))}
SUM_ORDERS = (0, 1, 2, 3)  # the emulation's realisations behind the norm-ratio envelope
# Rank 1's sweeps, per feature channel: scale and offset (signs and sizes differ per channel, so the first layers see another mixture, not a
# louder copy), and the coordinates with their axes permuted and stretched (the positional layers' relative coordinates change in kind).
# A uniform x3 + 2 left the local-BatchNorm control too close to the bounds (cosine median 0.990 at shift 6.0, norm-ratio quantile 0.075 at
# the rv-av2 widths: with the ReLU gates open the network is nearly affine and BatchNorm undoes a uniform scale); the ranks were made more
# different until the control missed every bound by the margin tests/test_two_rank_cpu.py states.
FEATURE_SCALE, FEATURE_OFFSET = (30.0, -25.0, 0.5, -40.0, 15.0), (10.0, -8.0, 0.5, 20.0, -15.0)
CART_AXES, CART_SCALE = (2, 0, 1), 6.0


def case_key(name: str, shift: float) -> str:
    return f"{name}/{shift}"


def rank_slices(name: str, world: int) -> List[Tuple[int, int]]:
    split, B = CASES[name][5], CASES[name][2]
    if world == 1:
        return [(0, B)]
    return [(0, split[0]), (split[0], B)]


def build_case(name: str, shift: float) -> dict:
    """Model (on the CPU, deterministic), its state dict, the heterogeneous batch and the functional's weights."""
    import torch

    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bench

    widths, n_cls, B, H, W, split, _ = CASES[name]
    if name == "c32":  # the model of test_gpu_model.py::test_detector_gradients_vs_oracle
        torch.manual_seed(0)
        backbone, head = bench.build_model("c32", n_cls)
        gen = torch.Generator().manual_seed(1)
        for m in list(backbone.modules()) + list(head.modules()):
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=gen)
                m.bias.data = 0.2 * torch.randn(m.bias.shape, generator=gen) + shift
        batch = bench.synthetic_batch(B, H, W, seed=5, device="cpu", n_cls=n_cls, boxes_per_sweep=6)
    else:  # the benchmarked widths, as tests/test_gpu_realwidth.py builds them
        from test_gpu_realwidth import _prepare

        backbone, head, _, batch = _prepare(widths, 5, n_cls, W, shift, B=B, H=H)
    sd = {**{f"backbone.{k}": v.clone() for k, v in backbone.state_dict().items()}, **{f"head.{k}": v.clone() for k, v in head.state_dict().items()}}
    lo = split[0]  # rank 1's sweeps: another sensor, as far as BatchNorm can tell
    features, cart, mask = batch["features"].clone(), batch["cart"].clone(), batch["mask"]
    scale, offset = torch.tensor(FEATURE_SCALE).view(1, -1, 1, 1), torch.tensor(FEATURE_OFFSET).view(1, -1, 1, 1)
    features[lo:] = (features[lo:] * scale + offset) * mask[lo:]
    cart[lo:] = cart[lo:][:, list(CART_AXES)] * CART_SCALE
    gen = torch.Generator().manual_seed(11)
    Rl, Rr = torch.randn(B, n_cls, H, W, generator=gen), torch.randn(B, 8, H, W, generator=gen)
    return {"name": name, "shift": shift, "widths": widths, "backbone": backbone, "head": head, "sd": sd, "features": features, "cart": cart, "mask": mask,
            "Rl": Rl, "Rr": Rr, "stem_type": "META", "pixels": H * W}


def functional(logits, reg, Rl, Rr, pixels: int):
    """L = (sum(logits * Rl) + sum(reg * Rr)) / (H * W): linear in the head outputs, so sum_r dL_r / dtheta under SyncBN is dL / dtheta
    of one model on all sweeps."""
    return ((logits.float() * Rl).sum() + (reg.float() * Rr).sum()) / pixels


def oracle_run(case: dict, nm, slices: Optional[Sequence[Tuple[int, int]]] = None):
    """The oracle with autograd on the whole batch -- or, ``slices``, once per slice with the slice's own BatchNorm statistics and the
    gradients summed (the local-BatchNorm control).  Returns (L, {parameter: gradient}, {running statistic: value})."""
    from oracle import model as om

    sd = case["sd"]
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
    B = case["features"].shape[0]
    total = 0.0
    for lo, hi in (slices or [(0, B)]):
        _, logits, reg = om.detector_forward(case["features"][lo:hi], case["cart"][lo:hi], {**sd, **params}, stem_type=case["stem_type"], nm=nm)
        loss = functional(logits, reg, case["Rl"][lo:hi], case["Rr"][lo:hi], case["pixels"])
        loss.backward()
        total += float(loss.detach())
    return total, {k: p.grad for k, p in params.items()}, dict(nm.running or {})


def fp32_numerics():
    from oracle import model as om

    return om.Numerics(train=True, running={})


# ------------------------------------------------------------------------------------------------------------------------------------
# yardstick arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def rel_err(a, b) -> float:
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def grad_metrics(g: Dict[str, "object"], g32: Dict[str, "object"]) -> dict:
    """Per parameter with |g32| >= 1e-9: cosine against fp32 and |log(|g| / |g32|)| (cosine cannot see a factor of the world size)."""
    import math

    import numpy as np

    cos, lr, names = [], [], []
    for k, ref in g32.items():
        n32 = float(ref.double().norm())
        if n32 < 1e-9:
            continue
        a, b = g[k].double().flatten().cpu(), ref.double().flatten()
        na = float(a.norm())
        cos.append(float((a @ b) / max(na * n32, 1e-300)))
        lr.append(abs(math.log(max(na, 1e-300) / n32)))
        names.append(k)
    cos, lr = np.array(cos), np.array(lr)
    worst = [(names[i], float(cos[i]), float(lr[i])) for i in np.argsort(cos)[:3]]
    return {"parameters": len(names), "median": float(np.median(cos)), "q05": float(np.quantile(cos, 0.05)), "min": float(cos.min()),
            "lr_q95": float(np.quantile(lr, 0.95)), "lr_max": float(lr.max()), "worst": worst}


# floors of test_gpu_model.py::test_detector_gradients_vs_oracle (median, 5 % quantile) for the well-conditioned regimes
FLOORS = {6.0: (0.995, 0.99), 3.0: (0.98, 0.9)}
MEDIAN_MARGIN, Q05_MARGIN, LOG_RATIO_MARGIN = 0.03, 0.05, 0.05  # the first two: that test's margins; the last: the issue's


def log_ratio_bound(yard: dict) -> float:
    """Envelope maximum of the emulation's own 95 % quantile of |log(|g16| / |g32|)| over its summation orders, + 0.05.  (A factor of
    two in a gradient is 0.69.)"""
    return max(r["lr_q95"] for r in yard["envelope"]) + LOG_RATIO_MARGIN


def gradient_violations(m: dict, yard: dict, shift: float) -> List[str]:
    """The gradient criteria a result misses (empty: inside the bounds)."""
    out = []
    emu = yard["emulation"]
    if not m["median"] >= emu["median"] - MEDIAN_MARGIN:
        out.append(f"cosine median {m['median']:.4f} < emulation {emu['median']:.4f} - {MEDIAN_MARGIN}")
    if not m["q05"] >= emu["q05"] - Q05_MARGIN:
        out.append(f"cosine 5 % quantile {m['q05']:.4f} < emulation {emu['q05']:.4f} - {Q05_MARGIN}")
    med_floor, q_floor = FLOORS[shift]
    if not (m["median"] > med_floor and m["q05"] > q_floor):
        out.append(f"cosine median {m['median']:.4f} / 5 % quantile {m['q05']:.4f} under the floors {med_floor} / {q_floor}")
    bound = log_ratio_bound(yard)
    if not m["lr_q95"] <= bound:
        out.append(f"95 % quantile of |log norm ratio| {m['lr_q95']:.4f} > {bound:.4f}")
    return out


def running_violations(running: Dict[str, "object"], running32: Dict[str, "object"], yard: dict) -> List[str]:
    """Running statistics against the fp32 oracle's, relative to the tensor maximum: 1.5 x (emulation vs fp32) + 1e-3 per tensor."""
    out = []
    for k, ref in running32.items():
        e, bound = rel_err(running[k].float().cpu(), ref), 1.5 * yard["running_err"][k] + 1e-3
        if not e <= bound:
            out.append(f"{k}: {e:.3e} > {bound:.3e}")
    return out


def load_yardstick() -> dict:
    import json

    with open(YARDSTICK) as f:
        return json.load(f)


def record_case(name: str, shift: float) -> dict:
    """The CPU side of one case (``emulation_yardstick.py two-rank``): fp32 oracle, bf16 emulation under ``SUM_ORDERS``, and the
    local-BatchNorm control of the inputs' discriminating power."""
    import torch
    from oracle import model as om

    case = build_case(name, shift)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    L32, g32, run32 = oracle_run(case, fp32_numerics())
    envelope, emu, running_err = [], None, None
    for order in SUM_ORDERS:
        L16, g16, run16 = oracle_run(case, om.Numerics.bf16(train=True, sum_order=order))
        m = grad_metrics(g16, g32)
        m.pop("worst")
        envelope.append({"sum_order": order, "L16": L16, **m})
        print("   ", envelope[-1], flush=True)
        if order == 0:
            emu, running_err = m, {k: rel_err(run16[k], v) for k, v in run32.items()}
    Lc, gc, _ = oracle_run(case, fp32_numerics(), rank_slices(name, 2))
    control = grad_metrics(gc, g32)
    control.pop("worst")
    print("    local-BatchNorm control", control, flush=True)
    return {"L32": L32, "parameters": emu["parameters"], "emulation": emu, "envelope": envelope, "running_err": running_err,
            "control_local_bn": {"L": Lc, **control}}
