"""``rv_head_final_bwd_sums`` / ``rv_head_final_bwd_apply`` (csrc/headfinal.hip) at the C ABI, against ``fused_bnb_ref.head_final_ref``.

The kernel recomputes ``dA = W^T dY`` by MFMA, gates it with ``scale*y+shift > 0``, sums ``g`` and ``g*y`` per pixel range, forms the final
conv's weight gradient through a wave-private LDS image read back transposed (inline ``ds_read_b64_tr_b16`` behind a hand-placed
``lgkmcnt`` wait), and in the apply pass writes ``dy = coef0*(g - coef1 - xhat*coef2)`` in a regrouped form.

Exact cases: integer ``y`` (-3..3), ``dY`` and ``W`` (-2..2), ``scale`` in {1/2, 1, 2}, integer ``shift`` / ``mean`` / ``coef1``, ``invstd`` /
``coef0`` / ``coef2`` signed powers of two in [1/4, 2].  Every term is an integer or a half-integer and ``exactness_margin`` (asserted on the
reference alone, first -- including the kernel's own grouping, sum |g*y| + |mean| sum |g|) stays below 2^23, so every fp32 partial sum is
exact in any order: sums, ``dW`` and ``dy`` (one rounding to the operand type) are compared with ``torch.equal``.  ``partial``,
``dw_partial``, ``dy`` and the pad columns of ``y`` / ``dY`` / ``dy`` are pre-filled with NaN.

What pins the kernel form: ``rv_head_final_bwd_rows(P)`` is asserted to be ``ceil(P / range)`` with ``range = 16 * ceil(ceil(P / 512) / 16)``
(restated here), at most 512, and every one of those rows must come back finite:

=====  =====  ====  ===============================================================================================
P      range  rows  reaches
=====  =====  ====  ===============================================================================================
1      16     1     one pixel: fifteen clamped (zeroed) lanes
15/17  16     1/2   a partial step; a second range of one pixel
16     16     1     exactly one full step
3000   16     188   a last range of eight pixels
8192   16     512   the largest row count
8193   32     257   the range-size step: two 16-pixel steps per range, a last range of one pixel
40000  80     500   five steps per range: the prefetch steady state of the loop
=====  =====  ====  ===============================================================================================

with ``c`` = 256 and 512 (``blockIdx.y == 1``), ``n_out`` = 1, 3, 26, 32, minimal strides and ``(c + 8, 40, c + 16)``, with and without
the ReLU, ``dw_partial`` given and NULL (the sums must be bit-identical), one fp16 case per kernel (the fp16-operand build), and argument
checks that must fail before any launch.

One real-valued case per kernel (``randn`` operands rounded to bf16, P = 3000, c = 512, ReLU): ``y`` is nudged to the nearest bf16 value
with ``|scale*y+shift| >= 1e-3`` (asserted on the reference; fewer than 1 % of the elements) so that the fp32 gate cannot differ from the
fp64 one.  Bounds, a priori: sums and ``dW`` ``|got - ref| <= (P + 8) * 2^-24 * sum |terms|`` per channel (any summation order);
``dy``: ``|got - ref| <= 2^-8 |ref| + 8 * 2^-24 * (|k0 g| + |cb y| + |ca|)`` -- one operand-type rounding plus the fp32 evaluation of
``k0*g + (cb*y + ca)``, ``ca = k0*(c2*mean*invstd - c1)``, ``cb = -k0*c2*invstd``.
"""

from __future__ import annotations

import functools

import pytest
import torch

import fused_bnb_ref as R
from test_gpu_forward import DEV
from test_gpu_tapconv4 import _ints

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROWS = {1: (16, 1), 15: (16, 1), 16: (16, 1), 17: (16, 2), 3000: (16, 188), 8192: (16, 512), 8193: (32, 257), 40000: (80, 500)}  # P: (range, rows)


def _expected_rows(P):
    rng = ((P + 511) // 512 + 15) // 16 * 16
    rows = (P + rng - 1) // rng
    assert rows <= 512 and ROWS.get(P, (rng, rows)) == (rng, rows)
    return rows


def _strides(c, padded):
    return (c + 8, 40, c + 16) if padded else (c, 32, c)


@functools.lru_cache(maxsize=None)
def _exact_case(P, c, n_out, relu, operand):
    """Integer operands and their fp64 reference, shared by the sums and the apply test of a case (and left unchanged)."""
    g = torch.Generator().manual_seed(P + c + n_out + relu)
    y, dY, W = _ints((P, c), g), _ints((P, n_out), g, -2, 3), _ints((n_out, c), g, -2, 3)
    scale, shift, mean, invstd, coef = R.head_bn(c, g)
    ref = R.head_final_ref(y, dY, W, scale, shift, mean, invstd, relu, coef=coef, operand=operand)
    R.assert_exact(R.exactness_margin(ref.g, ref.xhat, dY, ref.act, y, mean))  # (on the reference alone)
    return dict(y=y, dY=dY, W=W, scale=scale, shift=shift, mean=mean, invstd=invstd, coef=coef, ref=ref)


class _Device:
    """The operands of a case on the device: NaN pad columns in y and dY, zero channels n_out .. 31 in dY and the packed weight."""

    def __init__(self, o, c, n_out, padded, dtype):
        P = o["y"].shape[0]
        self.P, self.c, self.n_out, self.dtype = P, c, n_out, dtype
        self.ld_y, self.ld_dy, self.ld_out = _strides(c, padded)
        self.y = torch.full((P, self.ld_y), NAN, dtype=dtype, device=DEV)
        self.y[:, :c] = o["y"].to(DEV)
        self.dY = torch.full((P, self.ld_dy), NAN, dtype=dtype, device=DEV)
        self.dY[:, :32] = 0
        self.dY[:, :n_out] = o["dY"].to(DEV)
        self.wp = torch.zeros((c, 32), dtype=dtype, device=DEV)  # the packed scatter image [c][32]
        self.wp[:, :n_out] = o["W"].t().to(DEV)
        self.vec = [o[k].float().to(DEV) for k in ("scale", "shift", "mean", "invstd")]
        self.coef = o["coef"].float().contiguous().to(DEV) if o.get("coef") is not None else None

    def head(self):
        from range_view_3d_detection_amd import _lib as L

        return (self.P, self.c, L.ptr(self.y), self.ld_y, L.ptr(self.dY), self.ld_dy, L.ptr(self.wp),
                *[L.ptr(v) for v in self.vec])

    def sums(self, relu, with_dw):
        """-> (rows, partial [rows + scratch][2][c] on the CPU, dW [32][c] or None, dw_partial tail still NaN)"""
        from range_view_3d_detection_amd import _lib as L

        rows = L.load().rv_head_final_bwd_rows(self.P)
        partial = torch.full((rows + L.STATS_SCRATCH_ROWS, 2, self.c), NAN, dtype=torch.float32, device=DEV)
        dwp = torch.full((rows + L.STATS_SCRATCH_ROWS, 32 * self.c), NAN, dtype=torch.float32, device=DEV) if with_dw else None
        L.call("rv_head_final_bwd_sums", *self.head(), relu, L.ptr(partial), L.ptr(dwp), L.stream_ptr())
        dw, tail = None, True
        if with_dw:
            dw = torch.full((32, self.c), NAN, dtype=torch.float32, device=DEV)
            L.call("rv_reduce_rows", L.ptr(dwp), rows, 32 * self.c, L.ptr(dw), L.stream_ptr())
            torch.cuda.synchronize()
            assert bool(torch.isfinite(dwp[:rows]).all())
            dw, tail = dw.cpu(), bool(torch.isnan(dwp[rows:]).all())
        torch.cuda.synchronize()
        return rows, partial.cpu(), dw, tail

    def apply(self, relu):
        from range_view_3d_detection_amd import _lib as L

        dy = torch.full((self.P, self.ld_out), NAN, dtype=self.dtype, device=DEV)
        L.call("rv_head_final_bwd_apply", *self.head(), relu, L.ptr(self.coef), L.ptr(dy), self.ld_out, L.stream_ptr())
        torch.cuda.synchronize()
        return dy.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _check_sums_exact(o, dev, relu):
    ref, c, n_out = o["ref"], dev.c, dev.n_out
    rows, partial, dw, tail = dev.sums(relu, True)
    assert rows == _expected_rows(dev.P)
    assert bool(torch.isfinite(partial[:rows]).all()), int((~torch.isfinite(partial[:rows])).sum())
    got = partial[:rows].double().sum(0)
    assert torch.equal(got[0], ref.sum_g), float((got[0] - ref.sum_g).abs().max())
    assert torch.equal(got[1], ref.sum_gx), float((got[1] - ref.sum_gx).abs().max())
    assert bool(torch.isnan(partial[rows:]).all()) and tail
    assert torch.equal(dw[:n_out].double(), ref.dW), float((dw[:n_out].double() - ref.dW).abs().max())
    assert bool((dw[n_out:] == 0).all())
    rows2, partial2, _, _ = dev.sums(relu, False)  # dw_partial == NULL: the same sums, bit for bit
    assert rows2 == rows and torch.equal(_bits(partial2[:rows]), _bits(partial[:rows])) and bool(torch.isnan(partial2[rows:]).all())


def _check_apply_exact(o, dev, relu):
    dy = dev.apply(relu)
    want = o["ref"].dy.float().to(dev.dtype)  # (fp64 -> fp32 is exact for these values, next line: ONE rounding, to the operand type)
    assert torch.equal(o["ref"].dy.float().double(), o["ref"].dy)
    got = dy[:, : dev.c]
    # (compared as VALUES: where the result is zero the header's grouping gives -0 under a negative coef0 and the kernel's
    #  k0*g + (cb*y + ca) gives +0 -- the same number)
    assert bool(torch.isfinite(got).all()) and torch.equal(got.double(), want.double()), float((got.double() - want.double()).abs().max())
    assert bool(torch.isnan(dy[:, dev.c:]).all())


# (P, c, n_out, padded strides, relu): every value of every axis at least once
EXACT = [(1, 256, 1, False, 1), (15, 512, 3, True, 0), (16, 256, 32, True, 1), (17, 512, 26, False, 1), (3000, 256, 26, True, 1),
         (3000, 512, 3, False, 0), (8192, 256, 3, False, 1), (8193, 512, 32, True, 1), (40000, 512, 26, True, 1), (40000, 256, 1, False, 0)]


@pytest.mark.parametrize("P,c,n_out,padded,relu", EXACT)
def test_sums_and_weight_gradient_exact(P, c, n_out, padded, relu):
    o = _exact_case(P, c, n_out, relu, torch.bfloat16)
    _check_sums_exact(o, _Device(o, c, n_out, padded, torch.bfloat16), relu)


@pytest.mark.parametrize("P,c,n_out,padded,relu", EXACT)
def test_apply_exact(P, c, n_out, padded, relu):
    o = _exact_case(P, c, n_out, relu, torch.bfloat16)
    _check_apply_exact(o, _Device(o, c, n_out, padded, torch.bfloat16), relu)


def test_sums_exact_in_the_fp16_operand_build():
    from range_view_3d_detection_amd import _lib as L

    o = _exact_case(3000, 256, 26, 1, torch.float16)
    with L.operand("f16"):
        _check_sums_exact(o, _Device(o, 256, 26, True, torch.float16), 1)


def test_apply_exact_in_the_fp16_operand_build():
    from range_view_3d_detection_amd import _lib as L

    o = _exact_case(3000, 256, 26, 1, torch.float16)
    with L.operand("f16"):
        _check_apply_exact(o, _Device(o, 256, 26, True, torch.float16), 1)


# ---- real-valued operands ----------------------------------------------------------------------------------------------------------
def _step16(v, up):
    """The next representable value of a 16-bit float tensor towards +inf (up) or -inf."""
    b = v.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    o = torch.where(b >= 0x8000, -mag, mag) + (1 if up else -1)  # (sign-magnitude -> an ordinal)
    nb = torch.where(o < 0, (-o) | 0x8000, o)
    nb = torch.where(nb >= 0x8000, nb - 0x10000, nb)
    return nb.to(torch.int16).view(v.dtype)


def _nudge(y, scale, shift, dtype, eps=1e-3):
    """y (fp64 values of ``dtype``) with every element of |scale*y+shift| < eps moved to the nearest ``dtype`` value outside that band."""
    t = scale * y + shift
    bad = t.abs() < eps
    lo, hi = (-eps - shift) / scale, (eps - shift) / scale  # the band in y (scale > 0)
    lo, hi = (lo + 0 * y)[bad], (hi + 0 * y)[bad]
    dn = lo.float().to(dtype)
    dn = torch.where(dn.double() > lo, _step16(dn, False), dn).double()  # the largest value <= lo
    up = hi.float().to(dtype)
    up = torch.where(up.double() < hi, _step16(up, True), up).double()   # the smallest value >= hi
    out = y.clone()
    out[bad] = torch.where((y[bad] - dn).abs() <= (up - y[bad]).abs(), dn, up)
    return out, float(bad.double().mean())


@functools.lru_cache(maxsize=None)
def _real_case():
    gen = torch.Generator().manual_seed(2024)
    P, c, n_out, dtype = 3000, 512, 26, torch.bfloat16
    rnd = lambda t: t.to(dtype).double()
    scale = (0.5 + torch.rand(c, generator=gen)).double()
    shift = (0.3 * torch.randn(c, generator=gen)).double()
    mean = (0.1 * torch.randn(c, generator=gen)).double()
    invstd = (0.8 + 0.4 * torch.rand(c, generator=gen)).double()
    coef = torch.stack([0.5 + torch.rand(c, generator=gen), 0.3 * torch.randn(c, generator=gen), 0.3 * torch.randn(c, generator=gen)]).double()
    y, nudged = _nudge(rnd(torch.randn(P, c, generator=gen)), scale, shift, dtype)
    assert torch.equal(rnd(y.float()), y) and nudged < 0.01, nudged
    assert float((scale * y + shift).abs().min()) >= 1e-3  # (on the reference: the fp32 gate cannot flip)
    dY, W = rnd(torch.randn(P, n_out, generator=gen)), rnd(0.3 * torch.randn(n_out, c, generator=gen))
    ref = R.head_final_ref(y, dY, W, scale, shift, mean, invstd, 1, coef=coef, operand=dtype)
    return dict(y=y, dY=dY, W=W, scale=scale, shift=shift, mean=mean, invstd=invstd, coef=coef, ref=ref, P=P, c=c, n_out=n_out)


def test_sums_real_valued_within_the_a_priori_bound():
    o = _real_case()
    ref, P, n_out = o["ref"], o["P"], o["n_out"]
    rows, partial, dw, _ = _Device(o, o["c"], n_out, True, torch.bfloat16).sums(1, True)
    assert rows == _expected_rows(P) and bool(torch.isfinite(partial[:rows]).all())
    got = partial[:rows].double().sum(0)
    m = R.exactness_margin(ref.g, ref.xhat, o["dY"], ref.act)
    u = (P + 8) * 2.0 ** -24
    for name, err, bound in (("sum g", (got[0] - ref.sum_g).abs(), u * m["g"]), ("sum g*xhat", (got[1] - ref.sum_gx).abs(), u * m["gx"]),
                             ("dW", (dw[:n_out].double() - ref.dW).abs(), u * m["dw"])):
        print(f"{name}: worst error / bound = {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all()), (name, float((err / bound).max()))
    assert bool((dw[n_out:] == 0).all())


def test_apply_real_valued_within_the_a_priori_bound():
    o = _real_case()
    ref, c = o["ref"], o["c"]
    dy = _Device(o, c, o["n_out"], True, torch.bfloat16).apply(1)
    k0, c1, c2 = o["coef"]
    ca, cb = k0 * (c2 * o["mean"] * o["invstd"] - c1), -k0 * c2 * o["invstd"]
    bound = 2.0 ** -8 * ref.dy.abs() + 8 * 2.0 ** -24 * ((k0 * ref.g).abs() + (cb * o["y"]).abs() + ca.abs())
    err = (dy[:, :c].double() - ref.dy).abs()
    print(f"dy: worst error / bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool(torch.isnan(dy[:, c:]).all())


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,match", [("c", "multiple of 256"), ("ld_dy", "bad channel strides"), ("ld_out", "bad stride"), ("partial", "null partial")])
def test_bad_arguments_fail_before_any_launch(what, match):
    from range_view_3d_detection_amd import _lib as L

    P, c = 64, 256
    z16 = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=DEV)
    y, dY, wp = z16(P, c), z16(P, 32), z16(c, 32)
    vec = [torch.ones(c, device=DEV) for _ in range(4)]
    coef = torch.ones(3, c, device=DEV)
    partial = torch.full((1 + L.STATS_SCRATCH_ROWS, 2, c), NAN, device=DEV)
    dy = torch.full((P, c), NAN, dtype=torch.bfloat16, device=DEV)
    cc, ld_dy, ld_out = (128 if what == "c" else c), (24 if what == "ld_dy" else 32), (c - 8 if what == "ld_out" else c)
    head = (P, cc, L.ptr(y), c, L.ptr(dY), ld_dy, L.ptr(wp), *[L.ptr(v) for v in vec], 1)
    if what != "ld_out":
        with pytest.raises(L.RvError, match=match):
            L.call("rv_head_final_bwd_sums", *head, L.ptr(None if what == "partial" else partial), None, L.stream_ptr())
    if what != "partial":
        with pytest.raises(L.RvError, match=match):
            L.call("rv_head_final_bwd_apply", *head, L.ptr(coef), L.ptr(dy), ld_out, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(partial).all()) and bool(torch.isnan(dy).all())
