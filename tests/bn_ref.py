"""Plain references of the BatchNorm / element-wise passes (``rv_bn_finalize``, ``rv_bn_fold_eval``, ``rv_ew_combine``,
``rv_ew_mask_grad``, ``rv_bn_bwd_reduce`` / ``_finalize`` / ``_apply`` and their ``_pair`` forms), written from the formulas in
``include/rv3d.h`` with torch ops only -- no project kernel.  Activations are (pixels, c) tensors, per-channel constants (c,).

``dt`` is the dtype the formulas are evaluated in: ``torch.float64`` everywhere, except that the 256 MiB cases of
``test_gpu_bn_passes.py`` evaluate in ``torch.float32`` on the device, which is exact for that file's small-integer data.
"""

from __future__ import annotations

import torch

EW_RELU_A, EW_RELU_B, EW_RELU_OUT = 1, 2, 4  # RV_EW_RELU_*


def masked_grad(dout, out, y, scale, shift, relu_z, dt=torch.float64):
    """g = dOut * [out > 0 if out is given] * [scale*y+shift > 0 if relu_z]  (both gates strict)."""
    g = dout.to(dt)
    if out is not None:
        g = g * (out.to(dt) > 0)
    if relu_z:
        g = g * ((y.to(dt) * scale.to(dt) + shift.to(dt)) > 0)
    return g


def xhat(y, mean, invstd, dt=torch.float64):
    return (y.to(dt) - mean.to(dt)) * invstd.to(dt)


def bwd_sums(g, xh):
    """(sum g, sum g*xhat) over the pixels, in fp64."""
    return g.double().sum(0), (g.double() * xh.double()).sum(0)


def bwd_apply(g, xh, coef):
    """dY = k0 * (g - k1 - xhat * k2), coef = (3, c)."""
    k = coef.to(g.dtype)
    return k[0] * (g - k[1] - xh * k[2])


def dres(g, old=None):
    """dRes = g, or old + g with RV_BNB_RES_ACCUM."""
    return g if old is None else g + old.to(g.dtype)


def bwd_finalize(s0, s1, count, gamma, invstd, dgamma_old=None, dbeta_old=None):
    """(dgamma, dbeta, coef) from the fp64 totals: dgamma (+)= sum g*xhat, dbeta (+)= sum g, coef = (gamma*invstd, s0/n, s1/n)."""
    dgamma = s1 if dgamma_old is None else s1 + dgamma_old.double()
    dbeta = s0 if dbeta_old is None else s0 + dbeta_old.double()
    coef = torch.stack([gamma.double() * invstd.double(), s0 / count, s1 / count])
    return dgamma, dbeta, coef


def combine(a, a_scale, a_shift, b, b_scale, b_shift, flags, dt=torch.float64):
    """out = relu?( fa(a) + fb(b) ), f(x) = relu?(scale*x + shift) when the scale is given."""

    def f(x, sc, sh, relu):
        x = x.to(dt)
        if sc is not None:
            x = x * sc.to(dt) + sh.to(dt)
        return x.clamp_min(0) if relu else x

    r = f(a, a_scale, a_shift, flags & EW_RELU_A)
    if b is not None:
        r = r + f(b, b_scale, b_shift, flags & EW_RELU_B)
    return r.clamp_min(0) if flags & EW_RELU_OUT else r


def mask_grad(dout, out, old=None, dt=torch.float64):
    """d (+)= dOut * [out > 0 if out is given]."""
    g = dout.to(dt)
    if out is not None:
        g = g * (out.to(dt) > 0)
    return g if old is None else g + old.to(dt)


def bn_finalize(x, gamma, beta, eps, momentum, running_mean=None, running_var=None, count=None):
    """Training-mode BatchNorm statistics of x (pixels, c) in fp64: the batch mean and BIASED variance, then the header's formulas.
    ``eps`` / ``momentum`` are the fp32 values the C ABI receives.  ``count``: the element count behind the unbiased factor
    (default: the pixels of x)."""
    x = x.double()
    n = x.shape[0] if count is None else count
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    r = {"scale": scale, "shift": beta.double() - mean * scale, "mean": mean, "invstd": invstd}
    unbias = n / (n - 1.0) if n > 1 else 1.0
    if running_mean is not None:
        r["running_mean"] = (1.0 - momentum) * running_mean.double() + momentum * mean
    if running_var is not None:
        r["running_var"] = (1.0 - momentum) * running_var.double() + momentum * var * unbias
    return r


def bn_fold_eval(gamma, beta, running_mean, running_var, eps):
    scale = gamma.double() / torch.sqrt(running_var.double() + eps)
    return scale, beta.double() - running_mean.double() * scale


def f32_ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (ref fp64, got fp32)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    r32 = ref.float().abs()
    ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double().clamp_min(2.0 ** -149)
    return ((got.double() - ref).abs() / ulp).max().item()
