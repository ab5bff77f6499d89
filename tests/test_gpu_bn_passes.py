"""The bandwidth-bound BatchNorm and element-wise passes (``csrc/bnbwd.hip``, ``csrc/misc.hip``), every kernel form, against the
plain references of ``bn_ref.py``: exact checks with small-integer data.

Method of test_gpu_tapconv{2,4,5,6}.py / test_gpu_wgrad3.py.  The data (``_Data``) are small integers and powers of two, chosen so
that every intermediate is exact: |g * xhat| <= 64 in steps of 0.5, so a partial row (512 pixels) is an exact fp32 count of
half-units, the fp64 column totals are exact, every dY is at most 88 units of its step (8 significand bits: exact in bf16 and
fp16) and |dRes| <= 8.  The element-wise results must therefore equal the reference BIT FOR BIT (``torch.equal``) and the sums
exactly -- whatever the tiling or summation order.  The mask source holds zeros and scale*y+shift is exactly 0 on a few per cent of
the elements: both gates are pinned as strict.  All launches go through the C ABI (``L.call``); outputs are channel slices of wider
buffers pre-filled with a sentinel (with spare pixel rows behind), inputs are read dense, through pitched rows (ld = c + 8) and as a
slice at channel offset 8 of a 2c-wide buffer whose other channels hold garbage.

Every case first asserts the kernel form ``rv_ew_pass_info`` reports for its own shape -- the plan the entry point launches from --
so a threshold change cannot silently move a case onto another kernel.  Form -> case:

* comb (``ew_combine_kernel``, ``ew_mask_grad_kernel``) ......... test_small_shapes[combine|mask_grad-*], test_fp16_build_combine
  ... with a grid-stride tail (work > 2048 x 256 octets) ........ test_grid_stride_tails
* rows, non-temporal (``ew_combine_rows_kernel<true, HAS_B>``) ... test_cache_switch_combine (c = 512, 96, 2048; with and without b;
                                                                  one pixel fewer reports the comb)
* lean reduce (``bn_bwd_reduce_lean_kernel<OUT>``, ``bn_bwd_reduce2_lean_kernel``) ... test_small_shapes[reduce|reduce_pair-c<=1024],
                                                                  test_offset_switch[*-4095]
* octet reduce (``bn_bwd_reduce_kernel``, ``bn_bwd_reduce2_kernel``) ... test_small_shapes[reduce|reduce_pair-1056|2048],
                                                                  test_offset_switch[reduce-y|reduce_pair-y-4096]
* lean apply ``bn_bwd_apply_lean_kernel<F>``: F = 0, 2, 4, 6, 12, 14 ... test_apply_every_flag_form; F = 1, 3, 5, 7, 13, 15 ...
                                                                  test_cache_switch_apply[512-*] (non-temporal side)
* octet apply ``bn_bwd_apply_kernel<0>`` ........................ test_small_shapes[apply-1056|2048], test_offset_switch[apply-*-4096]
  ``bn_bwd_apply_kernel<1>`` (non-temporal) ..................... test_cache_switch_apply[2048-*]
* pair apply ``bn_bwd_apply2_kernel<0>`` / ``<1>`` ............... test_small_shapes[apply_pair-*] / test_cache_switch_apply_pair
* fused finalize (``bn_reduce_finalize_kernel``, ``bn_bwd_reduce_finalize_kernel``), rows <= 2048, and with the device-side
  count ......................................................... test_bn_finalize, test_bn_bwd_finalize, *_device_count
* two-stage finalize (``col_reduce_kernel`` + ``bn_finalize_kernel`` / ``bn_bwd_finalize_kernel``), rows 2049 and 4100 ... the same
* ``reduce_rows_kernel`` ....................................... test_reduce_rows
* thread layouts where the channel group does not divide 256 (c = 24, 96, 160: 252 / 240 / 240 active threads in the lean form,
  c = 96: 252 in the octet pair form) ........................... test_small_shapes[*-24|96|160]

The three passes meet through a real ``coef`` in test_chained_passes_on_random_data (random bf16 data, the closed form and the
bounds of test_gpu_backward.py::test_bn_backward_kernels_exact).  test_argument_checks pins the rejections.
"""

from __future__ import annotations

import pytest
import torch

import bn_ref as R
from test_gpu_forward import DEV, rel_err

pytestmark = pytest.mark.gpu

SENTINEL = 77.0  # canary value of everything a launch must not touch (exact in bf16 and fp16), as in test_gpu_tapconv2.py
GARBAGE = 99.0   # what the channels beside a pitched / sliced INPUT hold
SPARE = 3        # pixel rows behind `pixels` in every output buffer
BIG_PITCH = 524296  # row pitch of the 2^32-byte cases: 4095 px x 524296 x 2 B < 2^32 <= 4096 px x 524296 x 2 B
LAYOUTS = ("dense", "pitched", "offset")


def _L():
    from range_view_3d_detection_amd import _lib as L

    return L


# ------------------------------------------------------------------------------------------------------------------ data
class _Data:
    """The exact-integer operands of one (pixels, c) case, generated on the device: activations in the storage dtype, per-channel
    constants in fp32 (value ranges: the table of the module's method, see the docstring)."""

    def __init__(self, n, c, seed, dtype=torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.n, self.c, self.dtype = n, c, dtype

        def ints(lo, hi, shape):
            return torch.randint(lo, hi + 1, shape, generator=g, device=DEV, dtype=torch.int8)

        def pick(values, shape):
            return torch.tensor(values, device=DEV)[torch.randint(0, len(values), shape, generator=g, device=DEV)]

        act = lambda lo, hi: ints(lo, hi, (n, c)).to(dtype)
        self.dout, self.dres_old = act(-4, 4), act(-4, 4)
        self.y, self.yb = act(-6, 6), act(-6, 6)
        self.out = act(-2, 2)
        ch = lambda lo, hi: ints(lo, hi, (c,)).float()
        self.mean, self.mean_b = ch(-2, 2), ch(-2, 2)
        self.invstd, self.invstd_b = pick([0.5, 1.0, 2.0], (c,)), pick([0.5, 1.0, 2.0], (c,))
        self.scale, self.shift = pick([-2.0, -1.0, 1.0, 2.0], (c,)), ch(-4, 4)
        coef = lambda: torch.stack([pick([-2.0, -0.5, 0.5, 1.0, 2.0], (c,)), ch(-2, 2), pick([-1.0, -0.5, 0.0, 0.5, 1.0], (c,))]).contiguous()
        self.coef, self.coef_b = coef(), coef()
        # rv_ew_combine: a = y, b = yb in [-6, 6]; scales in {1, 2}, shifts in [-4, 4]
        self.sa, self.ta, self.sb, self.tb = ch(1, 2), ch(-4, 4), ch(1, 2), ch(-4, 4)
        self._placed = {}

    def op(self, name, layout="dense", n=None):
        """(view of the first n pixels, row pitch) of an activation in a layout; the channels beside it hold GARBAGE."""
        key = (name, layout)
        if key not in self._placed:
            t = getattr(self, name)
            if layout == "dense":
                self._placed[key] = (t, self.c)
            else:
                width, off = (self.c + 8, 0) if layout == "pitched" else (2 * self.c, 8)
                buf = torch.full((self.n, width), GARBAGE, dtype=self.dtype, device=DEV)
                buf[:, off:off + self.c] = t
                self._placed[key] = (buf[:, off:off + self.c], width)
        v, ld = self._placed[key]
        return v[: (n or self.n)], ld


_small_cache = {}


def _small(c, n=1537, dtype=torch.bfloat16):
    key = (c, n, dtype)
    if key not in _small_cache:
        _small_cache[key] = _Data(n, c, seed=1000 + c, dtype=dtype)
    return _small_cache[key]


_big_cache = {}


def _big(n, c):
    """The operands of a 256 MiB case: generated once, one such set alive at a time (about 1.3 GB)."""
    if (n, c) not in _big_cache:
        _big_cache.clear()
        torch.cuda.empty_cache()
        _big_cache[(n, c)] = _Data(n, c, seed=c)
    return _big_cache[(n, c)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _small_cache.clear()
    _big_cache.clear()
    torch.cuda.empty_cache()


class _Out:
    """An output: the channel slice [8, 8 + c) of a wider sentinel-filled buffer with SPARE pixel rows behind `n`."""

    def __init__(self, n, c, dtype, wide=True, init=None):
        self.n, self.c = n, c
        self.ld = 2 * c if wide else c + 16
        self.buf = torch.full((n + SPARE, self.ld), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[:n, 8:8 + c]
        if init is not None:
            self.view.copy_(init)

    def check(self, ref_fn, what, chunk_elems=1 << 24):
        """The slice equals ref_fn(p0, p1) (rounded once to the storage type) bit for bit; everything else is still the sentinel."""
        step = max(1, chunk_elems // self.c)
        for p0 in range(0, self.n, step):
            p1 = min(self.n, p0 + step)
            _assert_equal(self.view[p0:p1], ref_fn(p0, p1), what, p0)
        left, right, behind = self.buf[:, :8], self.buf[:, 8 + self.c:], self.buf[self.n:]
        assert bool((left == SENTINEL).all()) and bool((right == SENTINEL).all()) and bool((behind == SENTINEL).all()), f"{what}: wrote outside its slice"


def _assert_equal(got, ref, what, p0=0):
    ref_s = ref.to(got.dtype)
    assert torch.equal(ref_s.to(ref.dtype), ref), f"{what}: the reference itself is not exact in {got.dtype}"
    if torch.equal(got, ref_s):
        return
    bad = (got != ref_s) | got.isnan()
    px, ch = bad.nonzero(as_tuple=True)
    first = [(int(p) + p0, int(c), float(got[p, c]), float(ref_s[p, c])) for p, c in zip(px[:6].tolist(), ch[:6].tolist())]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; pixels {int(px.min()) + p0}..{int(px.max()) + p0}, "
                         f"channels {sorted(set(ch.tolist()))[:16]}; first (pixel, channel, got, want): {first}")


def _info(pass_id, n, c, ld=None, has_out=False, has_dres=False, flags=0):
    """rv_ew_pass_info; ld: the row pitches in the entry point's argument order, exactly as the launch will pass them."""
    return _L().ew_pass_info(pass_id, n, c, ld, has_out, has_dres, flags)


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ pass runners
def _run_reduce(D, n, layout, use_out, relu_z, expect_form, y_op=None):
    """rv_bn_bwd_reduce over the first n pixels of D: NaN-filled partial buffer, exact fp64 column totals."""
    L = _L()
    c = D.c
    (dout, ld_dout), (out, ld_out), (y, ld_y) = D.op("dout", layout, n), D.op("out", layout, n), y_op or D.op("y", layout, n)
    info = _info(L.EW_PASS_BWD_REDUCE, n, c, (ld_dout, ld_out, ld_y), use_out)
    rows = L.load().rv_bn_bwd_rows(n)
    assert rows == (n + 511) // 512
    assert info == (expect_form, 0, rows, 1 if (use_out and expect_form == L.EW_FORM_LEAN) else 0), info
    partial = torch.full((rows + L.STATS_SCRATCH_ROWS, 2, c), float("nan"), dtype=torch.float32, device=DEV)
    flags = L.BNB_RELU_Z if relu_z else 0
    L.call("rv_bn_bwd_reduce", n, c, L.ptr(dout), ld_dout, L.ptr(out) if use_out else None, ld_out, L.ptr(y), ld_y,
           L.ptr(D.scale), L.ptr(D.shift), L.ptr(D.mean), L.ptr(D.invstd), flags, L.ptr(partial), L.stream_ptr())
    _sync()
    g = R.masked_grad(D.dout[:n], D.out[:n] if use_out else None, D.y[:n], D.scale, D.shift, relu_z)
    s0, s1 = R.bwd_sums(g, R.xhat(D.y[:n], D.mean, D.invstd))
    _check_partial(partial, rows, s0, s1, f"reduce n={n} c={c} {layout} out={use_out} relu_z={relu_z}")


def _check_partial(partial, rows, s0, s1, what):
    assert bool(torch.isfinite(partial[:rows]).all()), f"{what}: a (row, channel) below rv_bn_bwd_rows was left unwritten"
    assert bool(partial[rows:].isnan().all()), f"{what}: wrote behind its rows"
    tot = partial[:rows].double().sum(0)
    assert torch.equal(tot[0], s0), f"{what}: sum g differs on channels {(tot[0] != s0).nonzero().flatten().tolist()[:16]}"
    assert torch.equal(tot[1], s1), f"{what}: sum g*xhat differs on channels {(tot[1] != s1).nonzero().flatten().tolist()[:16]}"


def _run_reduce_pair(D, n, layout, expect_form, ya_op=None):
    L = _L()
    c = D.c
    (dout, ld_dout), (out, ld_out), (ya, ld_ya), (yb, ld_yb) = D.op("dout", layout, n), D.op("out", layout, n), ya_op or D.op("y", layout, n), D.op("yb", layout, n)
    info = _info(L.EW_PASS_BWD_REDUCE_PAIR, n, c, (ld_dout, ld_out, ld_ya, ld_yb), True)
    rows = L.load().rv_bn_bwd_rows(n)
    assert info == (expect_form, 0, rows, 0), info
    pa, pb = (torch.full((rows + L.STATS_SCRATCH_ROWS, 2, c), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
    L.call("rv_bn_bwd_reduce_pair", n, c, L.ptr(dout), ld_dout, L.ptr(out), ld_out, L.ptr(ya), ld_ya, L.ptr(D.mean),
           L.ptr(D.invstd), L.ptr(yb), ld_yb, L.ptr(D.mean_b), L.ptr(D.invstd_b), L.ptr(pa), L.ptr(pb), L.stream_ptr())
    _sync()
    g = R.masked_grad(D.dout[:n], D.out[:n], None, None, None, False)
    what = f"reduce_pair n={n} c={c} {layout}"
    s0, s1a = R.bwd_sums(g, R.xhat(D.y[:n], D.mean, D.invstd))
    _check_partial(pa, rows, s0, s1a, what + " (a)")
    _, s1b = R.bwd_sums(g, R.xhat(D.yb[:n], D.mean_b, D.invstd_b))
    _check_partial(pb, rows, s0, s1b, what + " (b)")
    assert torch.equal(pa[:rows, 0], pb[:rows, 0]), what + ": the two sides' rows of sum g differ"


def _run_apply(D, n, layout, use_out, relu_z, dres_mode, expect, dt=torch.float64, wide=True, ops=None, outs=None):
    """rv_bn_bwd_apply.  dres_mode: None, "write" or "accum".  expect = (form, non-temporal); the template index follows from the
    arguments (lean: F; octet: MODE).  ops / outs: operands placed by the caller (the 2^32-byte cases)."""
    L = _L()
    c = D.c
    ops, outs = ops or {}, outs or {}
    (dout, ld_dout), (out, ld_out) = D.op("dout", layout, n), D.op("out", layout, n)
    y, ld_y = ops.get("y") or D.op("y", layout, n)
    dy = outs.get("dy") or _Out(n, c, D.dtype, wide)
    dr = None
    if dres_mode:
        dr = outs.get("dres") or _Out(n, c, D.dtype, wide)
        if dres_mode == "accum":
            dr.view.copy_(D.dres_old[:n])
    flags = (L.BNB_RELU_Z if relu_z else 0) | (L.BNB_RES_ACCUM if dres_mode == "accum" else 0)
    ld_out_arg, ld_dres_arg = (ld_out if use_out else 0), (dr.ld if dr else 0)
    info = _info(L.EW_PASS_BWD_APPLY, n, c, (ld_dout, ld_out_arg, ld_y, dy.ld, ld_dres_arg), use_out, dr is not None, flags)
    form, nt = expect
    if form == L.EW_FORM_LEAN:
        lanes = 256 // (c // 4)
        index = nt | (2 if use_out else 0) | (4 if dr else 0) | (8 if dres_mode == "accum" else 0)
    else:
        lanes, index = 256 // (c // 8), nt
    assert info == (form, nt, min(4096, (n + lanes - 1) // lanes), index), info
    L.call("rv_bn_bwd_apply", n, c, L.ptr(dout), ld_dout, L.ptr(out) if use_out else None, ld_out_arg, L.ptr(y), ld_y,
           L.ptr(D.scale), L.ptr(D.shift), L.ptr(D.mean), L.ptr(D.invstd), L.ptr(D.coef), flags, L.ptr(dy.view), dy.ld,
           L.ptr(dr.view) if dr else None, ld_dres_arg, L.stream_ptr())
    _sync()
    what = f"apply n={n} c={c} {layout} out={use_out} relu_z={relu_z} dres={dres_mode} F/MODE={index}"

    def g_of(p0, p1):
        return R.masked_grad(D.dout[p0:p1], D.out[p0:p1] if use_out else None, D.y[p0:p1], D.scale, D.shift, relu_z, dt)

    dy.check(lambda p0, p1: R.bwd_apply(g_of(p0, p1), R.xhat(D.y[p0:p1], D.mean, D.invstd, dt), D.coef), what + " dy")
    if dr:
        dr.check(lambda p0, p1: R.dres(g_of(p0, p1), D.dres_old[p0:p1] if dres_mode == "accum" else None), what + " dres")
    return info


def _run_apply_pair(D, n, layout, expect_nt, dt=torch.float64, wide=True):
    L = _L()
    c = D.c
    (dout, ld_dout), (out, ld_out), (ya, ld_ya), (yb, ld_yb) = D.op("dout", layout, n), D.op("out", layout, n), D.op("y", layout, n), D.op("yb", layout, n)
    dya, dyb = _Out(n, c, D.dtype, wide), _Out(n, c, D.dtype, wide)
    info = _info(L.EW_PASS_BWD_APPLY_PAIR, n, c, None, True)
    lanes = 256 // (c // 8)
    assert info == (L.EW_FORM_OCTET, expect_nt, min(4096, (n + lanes - 1) // lanes), expect_nt), info
    L.call("rv_bn_bwd_apply_pair", n, c, L.ptr(dout), ld_dout, L.ptr(out), ld_out, L.ptr(ya), ld_ya, L.ptr(D.mean),
           L.ptr(D.invstd), L.ptr(D.coef), L.ptr(dya.view), dya.ld, L.ptr(yb), ld_yb, L.ptr(D.mean_b), L.ptr(D.invstd_b), L.ptr(D.coef_b),
           L.ptr(dyb.view), dyb.ld, L.stream_ptr())
    _sync()
    g_of = lambda p0, p1: R.masked_grad(D.dout[p0:p1], D.out[p0:p1], None, None, None, False, dt)
    what = f"apply_pair n={n} c={c} {layout}"
    dya.check(lambda p0, p1: R.bwd_apply(g_of(p0, p1), R.xhat(D.y[p0:p1], D.mean, D.invstd, dt), D.coef), what + " dya")
    dyb.check(lambda p0, p1: R.bwd_apply(g_of(p0, p1), R.xhat(D.yb[p0:p1], D.mean_b, D.invstd_b, dt), D.coef_b), what + " dyb")


COMBINE_VARIANTS = [  # (b given, a affine, b affine, flags)
    (True, True, True, R.EW_RELU_A | R.EW_RELU_OUT), (True, True, False, R.EW_RELU_B), (False, True, False, R.EW_RELU_A), (True, False, True, R.EW_RELU_OUT),
    (False, False, False, 0), (True, True, True, R.EW_RELU_A | R.EW_RELU_B | R.EW_RELU_OUT)]


def _run_combine(D, n, layout, variant, expect, dt=torch.float64, wide=True):
    """rv_ew_combine.  expect = (form, non-temporal, grid)."""
    L = _L()
    c = D.c
    has_b, aff_a, aff_b, flags = variant
    (a, ld_a), (b, ld_b) = D.op("y", layout, n), D.op("yb", layout, n)
    o = _Out(n, c, D.dtype, wide)
    info = _info(L.EW_PASS_COMBINE, n, c, None, has_b)
    assert info == (*expect, 1 if (has_b and expect[0] == L.EW_FORM_ROWS) else 0), info
    sa, ta = (D.sa, D.ta) if aff_a else (None, None)
    sb, tb = (D.sb, D.tb) if (aff_b and has_b) else (None, None)
    L.call("rv_ew_combine", n, c, L.ptr(a), ld_a, L.ptr(sa), L.ptr(ta), L.ptr(b) if has_b else None, ld_b if has_b else 0,
           L.ptr(sb), L.ptr(tb), L.ptr(o.view), o.ld, flags, L.stream_ptr())
    _sync()
    o.check(lambda p0, p1: R.combine(D.y[p0:p1], sa, ta, D.yb[p0:p1] if has_b else None, sb, tb, flags, dt), f"combine n={n} c={c} {layout} {variant}")


def _run_mask_grad(D, n, layout, use_out, accumulate, expect_grid):
    L = _L()
    c = D.c
    (dout, ld_dout), (out, ld_out) = D.op("dout", layout, n), D.op("out", layout, n)
    d = _Out(n, c, D.dtype, init=D.dres_old[:n] if accumulate else None)
    info = _info(L.EW_PASS_MASK_GRAD, n, c, None, use_out)
    assert info == (L.EW_FORM_COMB, 0, expect_grid, 0), info
    L.call("rv_ew_mask_grad", n, c, L.ptr(dout), ld_dout, L.ptr(out) if use_out else None, ld_out if use_out else 0,
           L.ptr(d.view), d.ld, 1 if accumulate else 0, L.stream_ptr())
    _sync()
    d.check(lambda p0, p1: R.mask_grad(D.dout[p0:p1], D.out[p0:p1] if use_out else None, D.dres_old[p0:p1] if accumulate else None),
            f"mask_grad n={n} c={c} {layout} out={use_out} accumulate={accumulate}")


# ------------------------------------------------------------------------------------------------------------------ small shapes
CHANNELS = [8, 24, 32, 64, 96, 160, 256, 512, 1024, 1056, 2048]


def _pixel_counts(c):
    """1, the pixel-lane counts of c (lean: 256 // (c/4) lanes, octet: 256 // (c/8)) minus / plus one, and the 512-pixel row edges."""
    ns = {1, 511, 512, 513, 999, 1537}
    for lanes in (256 // (c // 4) if c <= 1024 else None, 256 // (c // 8)):
        if lanes:
            ns |= {lanes - 1, lanes, lanes + 1}
    return sorted(n for n in ns if n > 0)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("which", ["reduce", "reduce_pair", "apply", "apply_pair", "combine", "mask_grad"])
def test_small_shapes(which, c):
    """Every pass at every channel layout: c <= 1024 takes the lean forms (1024: one pixel lane), 1056 and 2048 the octet forms; pixel
    counts around the lane count of c and around the 512-pixel rows; the three input layouts and the option combinations rotate."""
    L = _L()
    D = _small(c)
    form = L.EW_FORM_LEAN if c <= 1024 else L.EW_FORM_OCTET
    for i, n in enumerate(_pixel_counts(c)):
        layout = LAYOUTS[(i + c // 8) % 3]
        if which == "reduce":
            for k in range(2):
                _run_reduce(D, n, layout, use_out=bool((i + k) & 1), relu_z=bool(k), expect_form=form)
        elif which == "reduce_pair":
            _run_reduce_pair(D, n, layout, form)
        elif which == "apply":
            _run_apply(D, n, layout, use_out=bool(i & 1), relu_z=bool(i & 2) or not (i & 1), dres_mode=(None, "write", "accum")[i % 3], expect=(form, 0))
        elif which == "apply_pair":
            _run_apply_pair(D, n, layout, 0)
        elif which == "combine":
            _run_combine(D, n, layout, COMBINE_VARIANTS[i % len(COMBINE_VARIANTS)], (L.EW_FORM_COMB, 0, (n * (c // 8) + 255) // 256))
        else:
            _run_mask_grad(D, n, layout, use_out=bool(i & 1), accumulate=bool(i & 2), expect_grid=(n * (c // 8) + 255) // 256)


@pytest.mark.parametrize("c,n", [(96, 999), (64, 513), (1056, 130)])
def test_apply_every_flag_form(c, n):
    """out in {NULL, given} x RV_BNB_RELU_Z x dres in {NULL, written, accumulated}: F = 0, 2, 4, 6, 12, 14 of the lean kernel (asserted
    from rv_ew_pass_info inside _run_apply), MODE 0 of the octet kernel at c = 1056."""
    L = _L()
    D = _small(c)
    seen = set()
    for use_out in (False, True):
        for relu_z in (False, True):
            for j, dres_mode in enumerate((None, "write", "accum")):
                info = _run_apply(D, n, LAYOUTS[(j + use_out) % 3], use_out, relu_z, dres_mode, (L.EW_FORM_LEAN if c <= 1024 else L.EW_FORM_OCTET, 0))
                seen.add(info[3])
    assert seen == ({0, 2, 4, 6, 12, 14} if c <= 1024 else {0})


def test_grid_stride_tails():
    """8 200 px x 512 channels = 524 800 octets, just over the 2048 x 256 items of one grid pass: the comb kernels loop."""
    L = _L()
    n, c = 8200, 512
    assert n * (c // 8) > 2048 * 256
    D = _small(c, n)
    for i, variant in enumerate(COMBINE_VARIANTS[:3]):
        _run_combine(D, n, LAYOUTS[i], variant, (L.EW_FORM_COMB, 0, 2048))
    for i, (use_out, accumulate) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        _run_mask_grad(D, n, LAYOUTS[i % 3], use_out, accumulate, 2048)


def test_fp16_build_combine():
    """The same source compiled with the other storage type (librv3d_hip_f16.so): rv_ew_combine at 999 x 96 with the same integers."""
    L = _L()
    with L.operand("f16"):
        D = _small(96, 999, torch.float16)
        for i, variant in enumerate(COMBINE_VARIANTS):
            _run_combine(D, 999, LAYOUTS[i % 3], variant, (L.EW_FORM_COMB, 0, (999 * 12 + 255) // 256))


# ------------------------------------------------------------------------------------------------------------------ the 256 MiB switch
# the smallest pixel count with pixels * c * 2 >= 2^28 and one fewer.  c = 96: the 4096-workgroup cap leaves trailing workgroups
# without any pixel (per = 342 -> 350 pixels per workgroup after rounding to the 10 / 21 lanes).  The reference runs on the device
# in fp32 (exact for these data), chunk by chunk.
SWITCH = [(512, 262144), (96, 1398102), (2048, 65536)]
F32 = torch.float32


def _sides(c, n):
    assert n * c * 2 >= 1 << 28 > (n - 1) * c * 2
    return ((n, 1), (n - 1, 0)) if c != 2048 else ((n, 1),)  # (c = 2048: the non-temporal octet forms; their MODE 0 runs in test_small_shapes)


@pytest.mark.parametrize("c,n", SWITCH)
def test_cache_switch_combine(c, n):
    L = _L()
    D = _big(n, c)
    lanes = 256 // (c // 8)
    for m, nt in _sides(c, n):
        for variant in (COMBINE_VARIANTS[0], COMBINE_VARIANTS[2]):  # with and without b
            expect = (L.EW_FORM_ROWS, 1, min(4096, (m + lanes - 1) // lanes)) if nt else (L.EW_FORM_COMB, 0, 2048)
            _run_combine(D, m, "dense", variant, expect, dt=F32, wide=False)


@pytest.mark.parametrize("c,n,use_out,dres_mode", [(512, 262144, o, d) for o in (False, True) for d in (None, "write", "accum")]
                         + [(96, 1398102, True, "accum"), (96, 1398102, False, "write"), (2048, 65536, True, "accum"), (2048, 65536, False, None)])
def test_cache_switch_apply(c, n, use_out, dres_mode):
    """Lean apply, both sides of the switch: the six out x dres combinations at c = 512 (F = 1, 3, 5, 7, 13, 15 and their even
    neighbours), one of them at c = 96; c = 2048: bn_bwd_apply_kernel<1>."""
    L = _L()
    D = _big(n, c)
    for m, nt in _sides(c, n):
        _run_apply(D, m, "dense", use_out, relu_z=True, dres_mode=dres_mode, expect=(L.EW_FORM_LEAN if c <= 1024 else L.EW_FORM_OCTET, nt), dt=F32, wide=False)


@pytest.mark.parametrize("c,n", SWITCH)
def test_cache_switch_apply_pair(c, n):
    D = _big(n, c)
    for m, nt in _sides(c, n):
        _run_apply_pair(D, m, "dense", nt, dt=F32, wide=False)


# ------------------------------------------------------------------------------------------------------------------ the 2^32-byte switch
@pytest.fixture(scope="module")
def giant():
    """4096 pixel rows of pitch BIG_PITCH (about 4.3 GB), never filled beyond the slices the cases use."""
    buf = torch.empty(4096 * BIG_PITCH, dtype=torch.bfloat16, device=DEV)
    yield buf.view(4096, BIG_PITCH)
    del buf
    torch.cuda.empty_cache()


class _GiantOut:
    """An output slice [8, 72) of the giant buffer; the eight channels on either side carry the sentinel."""

    def __init__(self, giant, n, c):
        self.n, self.c, self.ld = n, c, BIG_PITCH
        self.region = giant[:, :c + 16]
        self.region.fill_(SENTINEL)
        self.view = giant[:n, 8:8 + c]

    def check(self, ref_fn, what):
        _assert_equal(self.view, ref_fn(0, self.n), what)
        keep = self.region.clone()
        keep[:self.n, 8:8 + self.c] = SENTINEL
        assert bool((keep == SENTINEL).all()), f"{what}: wrote outside its slice"


@pytest.mark.parametrize("n", [4095, 4096])
@pytest.mark.parametrize("which,operand", [("reduce", "y"), ("reduce_pair", "y"), ("apply", "y"), ("apply", "dy"), ("apply", "dres")])
def test_offset_switch(giant, which, operand, n):
    """c = 64 with ONE operand at row pitch 524 296: 4095 pixels keep 32-bit byte offsets (lean form), 4096 do not (octet form);
    the large pitch on y, then on dy, then on dres -- every term of the guard's ld_max."""
    L = _L()
    c = 64
    D = _small(c, 4096)
    form = L.EW_FORM_LEAN if n == 4095 else L.EW_FORM_OCTET
    assert (n * BIG_PITCH * 2 < 1 << 32) == (n == 4095)
    y_op = None
    if operand == "y":
        giant[:, :c] = D.y
        y_op = (giant[:n, :c], BIG_PITCH)
    if which == "reduce":
        _run_reduce(D, n, "dense", use_out=True, relu_z=True, expect_form=form, y_op=y_op)
    elif which == "reduce_pair":
        _run_reduce_pair(D, n, "dense", form, ya_op=y_op)
    else:
        outs = {operand: _GiantOut(giant, n, c)} if operand != "y" else {}
        _run_apply(D, n, "dense", use_out=True, relu_z=True, dres_mode="accum" if operand == "dres" else "write", expect=(form, 0),
                   ops={"y": y_op} if y_op else None, outs=outs)


# ------------------------------------------------------------------------------------------------------------------ finalize passes
ROWS = [1, 15, 16, 17, 63, 64, 65, 2048, 2049, 4100]  # <= 2048: one launch; 2049, 4100: column reduction + finalize
FIN_CHANNELS = [8, 24, 40, 72, 256]  # none of the first four fills a 16-channel or a 64-channel block
PX_PER_ROW = 8
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the C ABI takes eps / momentum as fp32
MOMENTUM = 0.125
# Two fp32 ulps, derived: the kernel forms every result in fp64 and rounds it ONCE to fp32 (half an ulp); the reference's fp64 value
# differs from the kernel's by ~1e-15 relative (var as E[x^2] - mean^2 against the two-pass form: 4e-15 on these data), which can
# only move the result across a rounding tie -- one more ulp at the most.
FIN_ULPS = 2.0


def _partial_rows(x, rows):
    """partial[rows + scratch][2][c] of x (rows * PX_PER_ROW pixels, c): exact fp32 row sums and sums of squares; NaN scratch."""
    L = _L()
    c = x.shape[1]
    xr = x.double().view(rows, -1, c)
    partial = torch.full((rows + L.STATS_SCRATCH_ROWS, 2, c), float("nan"), dtype=torch.float32, device=DEV)
    partial[:rows, 0], partial[:rows, 1] = xr.sum(1).float(), (xr * xr).sum(1).float()
    assert torch.equal(partial[:rows, 1].double(), (xr * xr).sum(1))
    return partial


def _fin_form(rows):
    L = _L()
    return L.EW_FORM_FUSED_FINALIZE if rows <= 2048 else L.EW_FORM_TWO_STAGE


def _bn_finalize(partial, rows, c, count, gamma, beta, rm, rv, want_stats=True):
    L = _L()
    o = {k: torch.full((c + 8,), SENTINEL, dtype=torch.float32, device=DEV) for k in ("scale", "shift", "mean", "invstd")}
    opt = lambda t: L.ptr(t) if (t is not None and want_stats) else None
    L.call("rv_bn_finalize", L.ptr(partial), rows, c, count, L.ptr(gamma), L.ptr(beta), EPS, MOMENTUM, opt(rm), opt(rv),
           L.ptr(o["scale"]), L.ptr(o["shift"]), opt(o["mean"]), opt(o["invstd"]), L.stream_ptr())
    _sync()
    for k, t in o.items():
        assert bool((t[c:] == SENTINEL).all()), f"{k}: wrote behind channel {c}"
    return {k: t[:c] for k, t in o.items()}


def _check_fin(got, ref, keys, what):
    for k in keys:
        u = R.f32_ulps(got[k], ref[k])
        assert u <= FIN_ULPS, f"{what}: {k} is {u} fp32 ulps from the fp64 reference"


@pytest.mark.parametrize("c", FIN_CHANNELS)
def test_bn_finalize(c):
    """rv_bn_finalize from exact partial rows of x = integers in [-12, 12] + a per-channel offset; channel 1 is constant (var clamps
    at 0, invstd = 1/sqrt(eps)); every row count, both forms; all optional pointers given, then all NULL."""
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(c)
    rnd = lambda *s: torch.rand(s, generator=g, device=DEV)
    for rows in ROWS:
        n = rows * PX_PER_ROW
        x = torch.randint(-12, 13, (n, c), generator=g, device=DEV).double() + torch.randint(-20, 21, (c,), generator=g, device=DEV)
        x[:, 1] = 7.0
        gamma, beta, rm0, rv0 = rnd(c) + 0.5, rnd(c) - 0.5, rnd(c) * 4 - 2, rnd(c) + 0.5
        partial = _partial_rows(x, rows)
        info = _info(L.EW_PASS_BN_FINALIZE, rows, c)
        assert info == (_fin_form(rows), 0, (c + 15) // 16 if rows <= 2048 else (c + 63) // 64, 0), info
        ref = R.bn_finalize(x, gamma, beta, EPS, MOMENTUM, rm0, rv0)
        assert float(ref["invstd"][1]) == pytest.approx(EPS ** -0.5, rel=1e-12)  # (the constant channel: var = 0)
        rm, rv = rm0.clone(), rv0.clone()
        got = _bn_finalize(partial, rows, c, n, gamma, beta, rm, rv)
        got.update(running_mean=rm, running_var=rv)
        _check_fin(got, ref, ("scale", "shift", "mean", "invstd", "running_mean", "running_var"), f"rows={rows} c={c}")
        got = _bn_finalize(_partial_rows(x, rows), rows, c, n, gamma, beta, None, None, want_stats=False)  # every optional pointer NULL
        _check_fin(got, ref, ("scale", "shift"), f"rows={rows} c={c} (optional pointers NULL)")
        assert bool((got["mean"] == SENTINEL).all()) and bool((got["invstd"] == SENTINEL).all())


@pytest.mark.parametrize("c", [8, 72])
def test_bn_finalize_single_element_and_device_count(c):
    """count = 1 (variance 0, unbiased factor 1), and the device-side count of SyncBN: rows = 1, count < 0, the element count stored
    at partial[2c] behind the (2, c) totals, with its own unbiased factor n / (n - 1)."""
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(7 + c)
    rnd = lambda *s: torch.rand(s, generator=g, device=DEV)
    gamma, beta, rm0, rv0 = rnd(c) + 0.5, rnd(c) - 0.5, rnd(c) * 4 - 2, rnd(c) + 0.5
    for n in (1, 4000):
        x = torch.randint(-12, 13, (n, c), generator=g, device=DEV).double() + torch.randint(-20, 21, (c,), generator=g, device=DEV)
        ref = R.bn_finalize(x, gamma, beta, EPS, MOMENTUM, rm0, rv0)
        for device_count in (False, True):
            partial = torch.full((1 + L.STATS_SCRATCH_ROWS, 2, c), float("nan"), dtype=torch.float32, device=DEV)
            partial[0, 0], partial[0, 1] = x.sum(0).float(), (x * x).sum(0).float()
            if device_count:
                partial.view(-1)[2 * c] = float(n)
            info = _info(L.EW_PASS_BN_FINALIZE, 1, c, flags=1 if device_count else 0)
            assert info == (L.EW_FORM_FUSED_FINALIZE, 0, (c + 15) // 16, 1 if device_count else 0), info
            rm, rv = rm0.clone(), rv0.clone()
            got = _bn_finalize(partial, 1, c, -1 if device_count else n, gamma, beta, rm, rv)
            got.update(running_mean=rm, running_var=rv)
            _check_fin(got, ref, ("scale", "shift", "mean", "invstd", "running_mean", "running_var"), f"n={n} c={c} device_count={device_count}")


@pytest.mark.parametrize("c", FIN_CHANNELS)
def test_bn_fold_eval(c):
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(c)
    rnd = lambda *s: torch.rand(s, generator=g, device=DEV)
    gamma, beta, rm, rv = rnd(c) + 0.5, rnd(c) - 0.5, rnd(c) * 4 - 2, rnd(c) + 0.01
    scale, shift = (torch.full((c + 8,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2))
    L.call("rv_bn_fold_eval", c, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), EPS, L.ptr(scale), L.ptr(shift), L.stream_ptr())
    _sync()
    ref_scale, ref_shift = R.bn_fold_eval(gamma, beta, rm, rv, EPS)
    _check_fin({"scale": scale[:c], "shift": shift[:c]}, {"scale": ref_scale, "shift": ref_shift}, ("scale", "shift"), f"fold_eval c={c}")
    assert bool((scale[c:] == SENTINEL).all()) and bool((shift[c:] == SENTINEL).all())


def _bwd_partial(rows, c, g):
    """Integer partial rows (sum g, sum g*xhat) in [-50, 50] and their exact fp64 totals."""
    L = _L()
    partial = torch.full((rows + L.STATS_SCRATCH_ROWS, 2, c), float("nan"), dtype=torch.float32, device=DEV)
    partial[:rows] = torch.randint(-50, 51, (rows, 2, c), generator=g, device=DEV).float()
    tot = partial[:rows].double().sum(0)
    return partial, tot[0], tot[1]


def _check_bwd_finalize(partial, rows, c, count, count_arg, g, what):
    """dgamma / dbeta exact (fresh, accumulated onto integer gradients, NULL); coef[0] exact; coef[1], coef[2] within one fp32 ulp of
    the fp64 quotients (the kernel multiplies by the fp64 reciprocal: 1e-16 relative, then rounds once)."""
    L = _L()
    pow2 = lambda: torch.tensor([0.5, 1.0, 2.0, 4.0], device=DEV)[torch.randint(0, 4, (c,), generator=g, device=DEV)]
    gamma, invstd = pow2(), pow2()
    tot = partial[:rows].double().sum(0)
    for mode in ("fresh", "accumulate", "null"):
        old = torch.randint(-30, 31, (2, c), generator=g, device=DEV).float()
        dgamma, dbeta = (torch.full((c + 8,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2))
        dgamma[:c], dbeta[:c] = old[0], old[1]
        coef = torch.full((3 * c + 8,), SENTINEL, dtype=torch.float32, device=DEV)
        ref_dgamma, ref_dbeta, ref_coef = R.bwd_finalize(tot[0], tot[1], count, gamma, invstd, *((old[0], old[1]) if mode == "accumulate" else ()))
        L.call("rv_bn_bwd_finalize", L.ptr(partial), rows, c, count_arg, L.ptr(gamma), L.ptr(invstd),
               L.ptr(dgamma) if mode != "null" else None, L.ptr(dbeta) if mode != "null" else None, 1 if mode == "accumulate" else 0, L.ptr(coef),
               L.stream_ptr())
        _sync()
        w = f"{what} ({mode})"
        if mode == "null":
            assert torch.equal(dgamma[:c], old[0]) and torch.equal(dbeta[:c], old[1]), w
        else:
            assert torch.equal(dgamma[:c].double(), ref_dgamma), f"{w}: dgamma"
            assert torch.equal(dbeta[:c].double(), ref_dbeta), f"{w}: dbeta"
        assert bool((dgamma[c:] == SENTINEL).all()) and bool((dbeta[c:] == SENTINEL).all()) and bool((coef[3 * c:] == SENTINEL).all()), f"{w}: wrote behind channel {c}"
        k = coef[:3 * c].view(3, c)
        assert torch.equal(k[0].double(), ref_coef[0]), f"{w}: coef[0]"
        for j in (1, 2):
            u = R.f32_ulps(k[j], ref_coef[j])
            assert u <= 1.0, f"{w}: coef[{j}] is {u} fp32 ulps from the fp64 quotient"


@pytest.mark.parametrize("c", FIN_CHANNELS)
def test_bn_bwd_finalize(c):
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(100 + c)
    for rows in ROWS:
        partial, _, _ = _bwd_partial(rows, c, g)
        info = _info(L.EW_PASS_BWD_FINALIZE, rows, c)
        assert info == (_fin_form(rows), 0, (c + 15) // 16 if rows <= 2048 else (c + 63) // 64, 0), info
        count = rows * 512 - 3
        _check_bwd_finalize(partial, rows, c, count, count, g, f"bwd_finalize rows={rows} c={c}")


@pytest.mark.parametrize("c", [8, 72])
def test_bn_bwd_finalize_device_count(c):
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(200 + c)
    partial, _, _ = _bwd_partial(1, c, g)
    count = 12345
    partial.view(-1)[2 * c] = float(count)
    assert _info(L.EW_PASS_BWD_FINALIZE, 1, c, flags=1) == (L.EW_FORM_FUSED_FINALIZE, 0, (c + 15) // 16, 1)
    _check_bwd_finalize(partial, 1, c, count, -1, g, f"bwd_finalize device count c={c}")


@pytest.mark.parametrize("cols", [1, 15, 16, 17, 100, 32 * 64])
def test_reduce_rows(cols):
    """rv_reduce_rows / rv_reduce_rows_count on integer rows: exact column totals, out[cols] == count, out_copy given and NULL."""
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(cols)
    for rows in [r for r in ROWS if r <= 2049]:
        partial = torch.full((rows + L.STATS_SCRATCH_ROWS, cols), float("nan"), dtype=torch.float32, device=DEV)
        partial[:rows] = torch.randint(-100, 101, (rows, cols), generator=g, device=DEV).float()
        ref = partial[:rows].double().sum(0)
        new = lambda: torch.full((cols + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        out = new()
        L.call("rv_reduce_rows", L.ptr(partial), rows, cols, L.ptr(out), L.stream_ptr())
        _sync()
        assert torch.equal(out[:cols].double(), ref) and bool((out[cols:] == SENTINEL).all()), (rows, cols)
        for with_copy in (True, False):
            out, copy = new(), new()
            L.call("rv_reduce_rows_count", L.ptr(partial), rows, cols, float(rows * 512 - 1), L.ptr(out), L.ptr(copy) if with_copy else None,
                   L.stream_ptr())
            _sync()
            assert torch.equal(out[:cols].double(), ref) and float(out[cols]) == rows * 512 - 1 and bool((out[cols + 1:] == SENTINEL).all()), (rows, cols)
            if with_copy:
                assert torch.equal(copy[:cols].double(), ref) and bool((copy[cols:] == SENTINEL).all()), (rows, cols)
            else:
                assert bool((copy == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ the passes chained
@pytest.mark.parametrize("c", [96, 1056])
def test_chained_passes_on_random_data(c):
    """reduce -> finalize -> apply through a real coef on random bf16 data with pitched rows, against the closed form and with the bounds
    (1e-5 on the sums, 4e-3 = one bf16 ulp on dy) of test_gpu_backward.py::test_bn_backward_kernels_exact."""
    L = _L()
    g = torch.Generator(device=DEV).manual_seed(c)
    n = 3000
    rn = lambda *s: torch.randn(s, generator=g, device=DEV)

    def pitched(t):
        buf = torch.full((n, c + 8), GARBAGE, dtype=torch.bfloat16, device=DEV)
        buf[:, :c] = t
        return buf[:, :c]

    dout, y, out = pitched(rn(n, c).bfloat16()), pitched((rn(n, c) * 2 + 0.5).bfloat16()), pitched(rn(n, c).bfloat16())
    gamma, beta = torch.rand(c, generator=g, device=DEV) + 0.5, rn(c) * 0.3
    mean, var = y.float().mean(0), y.float().var(0, unbiased=False)
    invstd = torch.rsqrt(var + 1e-5)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    form = L.EW_FORM_LEAN if c <= 1024 else L.EW_FORM_OCTET
    ld = c + 8
    rows = L.load().rv_bn_bwd_rows(n)
    for flags, use_out in ((0, True), (L.BNB_RELU_Z, False), (L.BNB_RELU_Z, True), (0, False)):
        gg = R.masked_grad(dout, out if use_out else None, y, scale, shift, bool(flags))
        xh = R.xhat(y, mean, invstd)
        s0, s1 = R.bwd_sums(gg, xh)
        dy_ref = (gamma * invstd).double() * (gg - s0 / n - xh * s1 / n)
        assert _info(L.EW_PASS_BWD_REDUCE, n, c, (ld, ld, ld), use_out)[0] == form and _info(L.EW_PASS_BWD_FINALIZE, rows, c)[0] == L.EW_FORM_FUSED_FINALIZE
        assert _info(L.EW_PASS_BWD_APPLY, n, c, (ld, ld, ld, 2 * c, 0), use_out, False, flags)[:2] == (form, 0)
        partial = torch.empty((rows + L.STATS_SCRATCH_ROWS, 2, c), dtype=torch.float32, device=DEV)
        common = (n, c, L.ptr(dout), ld, L.ptr(out) if use_out else None, ld, L.ptr(y), ld, L.ptr(scale), L.ptr(shift),
                  L.ptr(mean), L.ptr(invstd))
        L.call("rv_bn_bwd_reduce", *common, flags, L.ptr(partial), L.stream_ptr())
        dgamma, dbeta, coef = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty((3, c), device=DEV)
        L.call("rv_bn_bwd_finalize", L.ptr(partial), rows, c, n, L.ptr(gamma), L.ptr(invstd), L.ptr(dgamma), L.ptr(dbeta), 0,
               L.ptr(coef), L.stream_ptr())
        dy = _Out(n, c, torch.bfloat16)
        L.call("rv_bn_bwd_apply", *common, L.ptr(coef), flags, L.ptr(dy.view), dy.ld, None, 0, L.stream_ptr())
        _sync()
        assert rel_err(dbeta, s0) < 1e-5 and rel_err(dgamma, s1) < 1e-5
        assert rel_err(dy.view.float(), dy_ref) < 4e-3  # one bf16 ulp


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    """rv_bn_bwd_reduce / _apply, rv_ew_combine and rv_ew_mask_grad reject what their _pair siblings reject -- pixels <= 0, c <= 0, a row
    pitch below c -- and, as before, c % 8, ld % 8, c > 2048 and a scale without its shift; nothing is launched (outputs untouched)."""
    L = _L()
    n, c = 40, 64
    big = lambda: torch.full((64, 4096), SENTINEL, dtype=torch.bfloat16, device=DEV)  # room for any of the rejected shapes
    src, dst = big(), big()
    partial = torch.full((8 + L.STATS_SCRATCH_ROWS, 2, 4096), SENTINEL, dtype=torch.float32, device=DEV)
    consts = torch.ones(3 * 4096, dtype=torch.float32, device=DEV)
    k = L.ptr(consts)

    def reduce(n=n, c=c, ld_dout=c, ld_out=c, ld_y=c, out=True):
        L.call("rv_bn_bwd_reduce", n, c, L.ptr(src), ld_dout, L.ptr(src) if out else None, ld_out, L.ptr(src), ld_y, k, k, k, k,
               0, L.ptr(partial), L.stream_ptr())

    def apply(n=n, c=c, ld_dout=c, ld_out=c, ld_y=c, ld_dy=c, ld_dres=c, out=True, dres=True):
        L.call("rv_bn_bwd_apply", n, c, L.ptr(src), ld_dout, L.ptr(src) if out else None, ld_out, L.ptr(src), ld_y, k, k, k, k, k,
               0, L.ptr(dst), ld_dy, L.ptr(dst) if dres else None, ld_dres, L.stream_ptr())

    def combine(n=n, c=c, ld_a=c, ld_b=c, ld_out=c, b=True, a_scale=True, a_shift=True, b_scale=True, b_shift=True):
        p = lambda on: k if on else None
        L.call("rv_ew_combine", n, c, L.ptr(src), ld_a, p(a_scale), p(a_shift), L.ptr(src) if b else None, ld_b, p(b_scale and b),
               p(b_shift and b), L.ptr(dst), ld_out, 0, L.stream_ptr())

    def mask_grad(n=n, c=c, ld_dout=c, ld_out=c, ld_d=c, out=True):
        L.call("rv_ew_mask_grad", n, c, L.ptr(src), ld_dout, L.ptr(src) if out else None, ld_out, L.ptr(dst), ld_d, 0,
               L.stream_ptr())

    bad = []
    for fn, lds in ((reduce, ("ld_dout", "ld_out", "ld_y")), (apply, ("ld_dout", "ld_out", "ld_y", "ld_dy", "ld_dres")),
                    (combine, ("ld_a", "ld_b", "ld_out")), (mask_grad, ("ld_dout", "ld_out", "ld_d"))):
        bad += [(fn, dict(n=0)), (fn, dict(n=-5)), (fn, dict(c=0)), (fn, dict(c=-8)), (fn, dict(c=12)), (fn, dict(c=60))]
        bad += [(fn, {ld: c - 8}) for ld in lds] + [(fn, {ld: c + 4}) for ld in lds]
    bad += [(reduce, dict(c=2056, ld_dout=2056, ld_out=2056, ld_y=2056)), (apply, dict(c=2056, ld_dout=2056, ld_out=2056, ld_y=2056, ld_dy=2056, ld_dres=2056))]
    bad += [(combine, dict(a_shift=False)), (combine, dict(a_scale=False)), (combine, dict(b_shift=False)), (combine, dict(b_scale=False))]
    for fn, kw in bad:
        with pytest.raises(L.RvError):
            fn(**kw)
    # the pair forms' own rule, unchanged
    for name in ("rv_bn_bwd_reduce_pair", "rv_bn_bwd_apply_pair"):
        for kw in (dict(n=0), dict(c=0), dict(c=12), dict(c=2056, ld=2056), dict(ld=c - 8), dict(ld=c + 4)):
            nn, cc = kw.get("n", n), kw.get("c", c)
            ld = kw.get("ld", cc)
            s = (L.ptr(src), ld)
            with pytest.raises(L.RvError):
                if name.endswith("reduce_pair"):
                    L.call(name, nn, cc, *s, *s, *s, k, k, *s, k, k, L.ptr(partial), L.ptr(partial), L.stream_ptr())
                else:
                    L.call(name, nn, cc, *s, *s, *s, k, k, k, L.ptr(dst), ld, *s, k, k, k, L.ptr(dst), ld, L.stream_ptr())
    _sync()
    assert bool((dst == SENTINEL).all()) and bool((partial == SENTINEL).all()), "a rejected call launched something"
    # an optional tensor that is NOT given may carry any pitch (the engine passes 0)
    reduce(out=False, ld_out=0)
    apply(out=False, ld_out=0, dres=False, ld_dres=0)
    combine(b=False, ld_b=0)
    mask_grad(out=False, ld_out=0)
    _sync()
