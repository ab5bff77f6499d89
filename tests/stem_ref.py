"""Plain references of the MetaKernel stem kernels -- the 9x-grid gathers of ``csrc/meta.hip``, the small-K layers of
``csrc/bnbwd.hip`` and the positional pair of ``csrc/posconv.hip`` -- written from the formulas in ``include/rv3d.h`` with torch ops
only: no project kernel, no tiling, no work order of any kernel.  Device-agnostic; everything is evaluated in fp64.

Layouts, as the kernels see them: ``feat`` / ``dfeat`` are (N*H*W, C); the 9x-grid tensors (``rel``, ``pos``, ``h1``, ``y2``, ``dy``) are
(N*H*W*9, channels) with row 9 p + k = tap k of pixel p; ``geo`` / ``dgeo`` are (N*H*W, 9*C) with channel k*C + c.  Tap k = 3 ky + kx is the
neighbour (h + ky - 1, w + kx - 1), zero outside the image (``F.unfold`` with padding 1).  Weights are the packed gather images
(c, ld_w) of which the columns below ``cin`` count; per-channel constants are (c,).  ``dims`` = (N, H, W).

A function that ends in a stored tensor returns the EXACT fp64 value; ``stored(x, dtype)`` rounds it once to the storage type.  Two
functions round on the way, as the kernels do: ``relative`` (the subtraction is one fp32 operation) and ``pos_forward`` /
``pos_modulate`` (the second layer multiplies the STORED h1; the modulation reads the STORED y2).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

import bn_ref as R

BNB_RELU_Z, BNB_Y_FROM_INPUT = 1, 4  # RV_BNB_*


def stored(x, dtype):
    """x rounded once to the storage type, as fp64 (exact when x fits fp32: the cast then rounds a single time)."""
    return x.to(dtype).double()


def gather9(x, dims):
    """x (N*H*W, C) -> (N*H*W, 9, C): tap k of pixel p is x at p's neighbour k, zeros outside the image."""
    n, h, w = dims
    xp = F.pad(x.reshape(n, h, w, -1), (0, 0, 1, 1, 1, 1))
    return torch.stack([xp[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 3).reshape(n * h * w, 9, -1)


def scatter9(t, dims):
    """The adjoint of gather9: t (N*H*W, 9, C) -> (N*H*W, C), out[q] = sum over the (p, k) whose neighbour k is q."""
    n, h, w = dims
    t = t.reshape(n, h, w, 9, -1)
    out = t.new_zeros(n, h + 2, w + 2, t.shape[-1])
    for ky in range(3):
        for kx in range(3):
            out[:, ky:ky + h, kx:kx + w] += t[:, :, :, 3 * ky + kx]
    return out[:, 1:-1, 1:-1].reshape(n * h * w, -1)


# ------------------------------------------------------------------------------------------------------------------ meta.hip
def relative(cart, dtype=torch.bfloat16, channels=32):
    """rel[p, k, 0:3] = cart[neighbour k of p] (0 outside) - cart[p] of an fp32 NCHW ``cart`` (N, 3, H, W): ONE fp32 subtraction, then
    one rounding to ``dtype``; channels 3.. are zero.  Returns (N*H*W*9, channels) fp64."""
    n, _, h, w = cart.shape
    c = cart.float().permute(0, 2, 3, 1).reshape(n * h * w, 3)
    d = gather9(c, (n, h, w)) - c[:, None]  # fp32
    rel = torch.zeros(n * h * w * 9, channels, dtype=torch.float64, device=cart.device)
    rel[:, :3] = d.reshape(-1, 3).to(dtype).double()
    return rel


def _act(pos, scale, shift):
    return pos.double() * scale.double() + shift.double()


def modulate(pos, scale, shift, feat, dims):
    """geo[p][k*C + c] = relu(scale*pos[9p + k] + shift) * feat[neighbour k of p]."""
    px = feat.shape[0]
    a = _act(pos, scale, shift).clamp_min(0).reshape(px, 9, -1)
    return (a * gather9(feat.double(), dims)).reshape(px, -1)


def modulate_bwd(dgeo, pos, scale, shift, feat, dims):
    """(dpos_act, dfeat) of rv_meta_modulate_bwd: dpos_act = dgeo * feat[neighbour], dfeat = adjoint gather of dgeo * relu(...)."""
    px = feat.shape[0]
    g = dgeo.double().reshape(px, 9, -1)
    a = _act(pos, scale, shift).clamp_min(0).reshape(px, 9, -1)
    return (g * gather9(feat.double(), dims)).reshape(px * 9, -1), scatter9(g * a, dims)


def modulate_z(dgeo, pos, scale, shift, feat, dims):
    """z = dgeo * feat[neighbour] * [scale*y + shift > 0] (strict) on the 9x grid."""
    px = feat.shape[0]
    z = dgeo.double().reshape(px, 9, -1) * gather9(feat.double(), dims)
    return z.reshape(px * 9, -1) * (_act(pos, scale, shift) > 0)


def modulate_bwd_sums(dgeo, pos, scale, shift, mean, invstd, feat, dims):
    """(S0, S1, dfeat): S0 = sum z, S1 = sum z * xhat over the 9x grid."""
    z = modulate_z(dgeo, pos, scale, shift, feat, dims)
    return z.sum(0), (z * R.xhat(pos, mean, invstd)).sum(0), modulate_bwd(dgeo, pos, scale, shift, feat, dims)[1]


def modulate_bwd_apply(dgeo, pos, scale, shift, mean, invstd, coef, feat, dims):
    """dy = coef0 (z - coef1 - xhat coef2)."""
    return R.bwd_apply(modulate_z(dgeo, pos, scale, shift, feat, dims), R.xhat(pos, mean, invstd), coef.double())


# ------------------------------------------------------------------------------------------------------------------ small-K layers
def smallk_y(v, w, cin):
    """The raw conv output y = W v of a 1x1 conv over the first ``cin`` stored channels."""
    return v[:, :cin].double() @ w[:, :cin].double().t()


def smallk_moments(v, cin_pad):
    """(m1, M2) = (sum v, sum v v^T) over the first cin_pad STORED channels (whatever the channels cin.. hold)."""
    x = v[:, :cin_pad].double()
    return x.sum(0), x.t() @ x


def smallk_stats(v, w, cin, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """Training-mode BatchNorm of y = W v, DIRECTLY from y (bn_ref.bn_finalize): scale, shift, mean, invstd, running_*."""
    return R.bn_finalize(smallk_y(v, w, cin), gamma, beta, eps, momentum, running_mean, running_var)


def smallk_apply(v, w, cin, scale, shift, relu):
    h = smallk_y(v, w, cin) * scale.double() + shift.double()
    return h.clamp_min(0) if relu else h


def smallk_bwd_planes(dout, out, y, v, w, cin, cin_pad, scale, shift, mean, invstd, flags):
    """(S0, S1, R (cin_pad, c)) of rv_bn_bwd_smallk_sums: g = masked_grad (both gates strict), R[d] = sum g v_d.  With
    RV_BNB_Y_FROM_INPUT y is W v itself (gate and xhat from the unrounded value), otherwise the stored ``y``.  Also returns g."""
    yy = smallk_y(v, w, cin) if flags & BNB_Y_FROM_INPUT else y.double()
    g = R.masked_grad(dout, out, yy, scale, shift, bool(flags & BNB_RELU_Z))
    s0, s1 = R.bwd_sums(g, R.xhat(yy, mean, invstd))
    return s0, s1, v[:, :cin_pad].double().t() @ g, g


def smallk_grads(g, y, v, cin, gamma, mean, invstd, global_s01=None, count=None):
    """(dgamma, dbeta, dW (c, cin)) from the definition: dy = k0 (g - k1 - xhat k2), dW[c][d] = sum_p dy[p, c] v[p, d], with
    k0 = gamma invstd, (k1, k2) = (sum g, sum g xhat) / count -- of ``global_s01`` (2, c) and a global ``count`` under SyncBN."""
    xh = R.xhat(y, mean, invstd)
    s0, s1 = R.bwd_sums(g, xh)
    n = g.shape[0] if count is None else count
    k1, k2 = (s0 / n, s1 / n) if global_s01 is None else (global_s01[0].double() / n, global_s01[1].double() / n)
    dy = gamma.double() * invstd.double() * (g - k1 - xh * k2)
    return s1, s0, dy.t() @ v[:, :cin].double()


# ------------------------------------------------------------------------------------------------------------------ positional pair
def pos_forward(rel, w1, cin, s1, t1, w2, dtype=torch.bfloat16):
    """(h1, y2, sum, sumsq): h1 = relu(s1 (W1 rel) + t1) exact; y2 = W2 stored(h1) exact and UNROUNDED; its column sums."""
    h1 = smallk_apply(rel, w1, cin, s1, t1, True)
    y2 = stored(h1, dtype) @ w2.double().t()
    return h1, y2, y2.sum(0), (y2 * y2).sum(0)


def pos_modulate(rel, w1, cin, s1, t1, w2, s2, t2, feat, dims, dtype=torch.bfloat16):
    """The inference form: modulate(stored(y2), s2, t2, feat)."""
    return modulate(stored(pos_forward(rel, w1, cin, s1, t1, w2, dtype)[1], dtype), s2, t2, feat, dims)


def pos_masked_grad(dy2, w2_scatter, rel, w1, cin, s1, t1):
    """(g, y1): dh1 = dy2 W2 (w2_scatter is W2 transposed: [ci][co]) gated by s1 y1 + t1 > 0 on the exact y1 = W1 rel."""
    y1 = smallk_y(rel, w1, cin)
    return (dy2.double() @ w2_scatter.double().t()) * (_act(y1, s1, t1) > 0), y1


def pos_backward_planes(dy2, w2_scatter, rel, w1, cin, s1, t1, mean1, invstd1):
    """(S0, S1, R[0:3] (3, C)) of rv_pos_backward_sums (rel channels cin..2 enter R as stored)."""
    g, y1 = pos_masked_grad(dy2, w2_scatter, rel, w1, cin, s1, t1)
    s0, s1_ = R.bwd_sums(g, R.xhat(y1, mean1, invstd1))
    return s0, s1_, rel[:, :3].double().t() @ g
