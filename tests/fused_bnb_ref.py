"""fp64 restatement of the two kernel families that form the BatchNorm-backward sums inside another kernel (include/rv3d.h):

* ``rv_tap_data_grad_bnb`` -- the backward-data launch of the conv BEHIND a BatchNorm(+ReLU): from the 16-bit values ``dx`` it stores,
  ``g = dx * [scale*y+shift > 0]`` (strict), ``sum g`` and ``sum g*xhat`` per channel, ``xhat = (y-mean)*invstd``;
* ``rv_head_final_bwd_sums`` / ``_apply`` -- a tower's final 1x1 conv fused with the BatchNorm(+ReLU) backward in front of it:
  ``dA = dY @ W`` recomputed, the same two sums, the final conv's weight gradient ``dW[o][c] = sum_px dY[px][o] * act[px][c]`` with
  ``act = relu?(scale*y+shift)`` rounded to the operand type (as the kernel packs it for the MFMA), and
  ``dy = coef0*(g - coef1 - xhat*coef2)`` exactly as the header writes it.

Plain torch in fp64, no device code, nothing of the library: tests/test_fused_bnb_ref_cpu.py checks it against autograd, the GPU tests
(test_gpu_tap_bnb_epilogue.py, test_gpu_head_final_kernels.py) hold the kernels to it.  Every tensor is channel-last: ``(..., C)``, the
per-channel vectors ``(C,)``; sums run over all leading dimensions.

``exactness_margin``: the exact tests feed small integers (scales and invstd in {1/2, 1, 2}), so every term a kernel adds up is an
integer or a half-integer; when the sum of the ABSOLUTE values of the terms of a channel stays below 2^23, every partial sum of those
terms -- in any order, grouped in any way -- is a multiple of 1/2 below 2^23, has 24 significant bits at most and is therefore formed in
fp32 without rounding.  (rv_head_final_bwd_sums adds up g*y, integers, and multiplies by invstd once at the end: there invstd may be any
power of two, and the margin to hold is ``gy``.)  The tests assert the margins on the reference alone; the comparison with the kernel
then is ``torch.equal``.
"""

from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch

EXACT_BELOW = float(2 ** 23)


def _f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().double().cpu()


def _lead(t: torch.Tensor):
    return tuple(range(t.dim() - 1))


def gate(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, relu: bool) -> torch.Tensor:
    """[scale*y+shift > 0] as fp64 0/1 (all ones without a ReLU)."""
    y = _f64(y)
    if not relu:
        return torch.ones_like(y)
    return ((_f64(scale) * y + _f64(shift)) > 0).double()


def data_grad_bnb_ref(dx_stored, y, scale, shift, mean, invstd, relu_z):
    """(sum g, sum g*xhat) per channel of ``rv_tap_data_grad_bnb``; ``dx_stored``: the 16-bit values the launch stores, taken as fp64."""
    dx, y = _f64(dx_stored), _f64(y)
    g = dx * gate(y, scale, shift, bool(relu_z))
    xhat = (y - _f64(mean)) * _f64(invstd)
    return g.sum(_lead(g)), (g * xhat).sum(_lead(g))


class HeadFinal(NamedTuple):
    dA: torch.Tensor      # (P, C)  dY @ W
    g: torch.Tensor       # (P, C)  dA * gate
    xhat: torch.Tensor    # (P, C)
    act: torch.Tensor     # (P, C)  relu?(scale*y+shift) rounded to the operand type
    sum_g: torch.Tensor   # (C,)
    sum_gx: torch.Tensor  # (C,)
    dW: torch.Tensor      # (n_out, C)
    dy: Optional[torch.Tensor]  # (P, C) fp64, NOT rounded (coef given), else None


def head_final_ref(y, dY, W, scale, shift, mean, invstd, relu, coef=None, operand: Optional[torch.dtype] = torch.bfloat16) -> HeadFinal:
    """y (P, C), dY (P, n_out), W (n_out, C): the final conv's weight.  ``operand``: the 16-bit type ``act`` is rounded to (None: kept
    in fp64 -- the autograd comparison).  ``coef`` (3, C) = rv_bn_bwd_finalize's (gamma*invstd, mean g, mean g*xhat)."""
    y, dY, W = _f64(y), _f64(dY), _f64(W)
    scale, shift, mean, invstd = _f64(scale), _f64(shift), _f64(mean), _f64(invstd)
    t = scale * y + shift
    dA = dY @ W
    g = dA * gate(y, scale, shift, bool(relu))
    xhat = (y - mean) * invstd
    act = t.clamp_min(0) if relu else t
    if operand is not None:
        act = act.float().to(operand).double()
    dW = dY.t() @ act
    dy = None
    if coef is not None:
        coef = _f64(coef)
        dy = coef[0] * (g - coef[1] - xhat * coef[2])
    return HeadFinal(dA, g, xhat, act, g.sum(0), (g * xhat).sum(0), dW, dy)


def exactness_margin(g, xhat, dY=None, act=None, y=None, mean=None) -> Dict[str, torch.Tensor]:
    """Per-channel sums of the absolute values of the terms the kernels add up:

    ``g``: sum |g|;  ``gx``: sum |g*xhat|;  ``dw`` (dY and act given): sum_px |dY[px][o]| * |act[px][c]|, (n_out, C);
    ``gy`` (y and mean given): sum |g*y| + |mean| * sum |g| -- rv_head_final_bwd_sums accumulates sum g*y and forms
    invstd * (sum g*y - mean * sum g) at the end, so its intermediate values are these, not those of ``gx``."""
    g, xhat = _f64(g), _f64(xhat)
    lead = _lead(g)
    out = {"g": g.abs().sum(lead), "gx": (g * xhat).abs().sum(lead)}
    if dY is not None and act is not None:
        dY, act = _f64(dY), _f64(act)
        out["dw"] = dY.abs().reshape(-1, dY.shape[-1]).t() @ act.abs().reshape(-1, act.shape[-1])
    if y is not None and mean is not None:
        out["gy"] = (g * _f64(y)).abs().sum(lead) + _f64(mean).abs() * out["g"]
    return out


def worst_margin(margin: Dict[str, torch.Tensor]) -> float:
    return max(float(v.max()) for v in margin.values())


def assert_exact(margin: Dict[str, torch.Tensor]) -> None:
    """Every sum of absolute terms below 2^23: see the module docstring."""
    for k, v in margin.items():
        assert float(v.max()) < EXACT_BELOW, (k, float(v.max()))


# ---- the per-channel operands of the exact tests (fp64; the GPU tests convert) ----------------------------------------------------
def pick(values, n: int, gen: torch.Generator) -> torch.Tensor:
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), (n,), generator=gen)]


SIGNED_POW2 = [s * p for s in (-1.0, 1.0) for p in (0.25, 0.5, 1.0, 2.0)]


def data_grad_bn(c: int, gen: torch.Generator):
    """(scale, shift, mean, invstd) of the rv_tap_data_grad_bnb tests: scale in {1/2, 1, 2}, integer shift (so that t == 0 occurs),
    integer mean in -1..1, invstd in {1/2, 1}."""
    return (pick([0.5, 1.0, 2.0], c, gen), torch.randint(-2, 3, (c,), generator=gen).double(), torch.randint(-1, 2, (c,), generator=gen).double(),
            pick([0.5, 1.0], c, gen))


def head_bn(c: int, gen: torch.Generator):
    """(scale, shift, mean, invstd, coef) of the exact head-final tests: as above, invstd / coef0 / coef2 signed powers of two in
    [1/4, 2], coef1 an integer."""
    coef = torch.stack([pick(SIGNED_POW2, c, gen), torch.randint(-3, 4, (c,), generator=gen).double(), pick(SIGNED_POW2, c, gen)])
    return (pick([0.5, 1.0, 2.0], c, gen), torch.randint(-2, 3, (c,), generator=gen).double(), torch.randint(-1, 2, (c,), generator=gen).double(),
            pick(SIGNED_POW2, c, gen), coef)
