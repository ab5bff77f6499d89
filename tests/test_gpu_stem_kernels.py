"""The MetaKernel stem kernels -- the 9x-grid gathers (``csrc/meta.hip``), the small-K layers (``csrc/bnbwd.hip``) and the positional
pair (``csrc/posconv.hip``) -- against the plain fp64 references of ``stem_ref.py``: exact checks through the C ABI.

Method of test_gpu_bn_passes.py.  DATA RULE: the inputs are small integers, halves and powers of two, chosen so that every fp32
intermediate is exact whatever the summation order or FMA contraction.  An element-wise output is then the exact value rounded ONCE to
the storage type and must equal the reference BIT FOR BIT (``torch.equal``); sums are compared with ``==`` in fp64.  The preconditions
are asserted from the data alone, before any launch: the exact result fits fp32 (``_eq``), and for every partial-sum output
max |term| x (terms one partial row can cover, from the documented row count) / unit < 2^24 (``_row_sums_exact``).  Value ranges:

* gathers: pos in [-6, 6], scale in {-1, 0.5, 1, 2}, shift in [-4, 4] (scale*pos + shift in halves, exactly 0 on a few per cent:
  the gates are pinned as strict), feat in [-4, 4], dgeo in [-3, 3], mean in halves of [-2, 2], invstd in {0.5, 1, 2}, coef as
  test_gpu_bn_passes.py.  |z xhat| <= 192 in quarters, 4608 terms per 512-pixel row; every element-wise result has at most 8
  significant bits.  The "fine" data (feat in eighths up to 63/8, dgeo in quarters up to 31/4, shift in quarters up to 4) push geo,
  dpos_act, dfeat and dy BEYOND 8 significant bits (13 for geo: beyond fp16's 11 too), ties included: round-to-nearest-even is what
  passes.  Their sums would not be exact in fp32 and are not compared.
* small-K: v in [-3, 3], w in {-1, 0, 1} (column 0 never 0), dout in [-4, 4], out in [-2, 2], stored y in [-6, 6]; eval scale in
  {-1, 0.5, 1, 2}, shift in halves -- or in 64ths ("fine": h beyond 8 bits).  Channels cin..7 of v hold finite GARBAGE against zero
  weight columns (the precondition written down in include/rv3d.h); the statistics / from-sums launches, which read no column at or
  beyond cin, get GARBAGE there too, and the statistics-only launch NaN in the moments of the channels at and beyond cin.
* positional pair: rel in [-3, 3], w1 in {-1, 0, 1}, s1 in {0.5, 1}, t1 in halves of [-2, 2], w2 in {-1, 0, 1} at density 1/8, dy2 in
  [-2, 2], mean1 in halves, invstd1 in {0.5, 1, 2}: h1 <= 11, |y2| <= 57 in halves, first-layer gates exactly 0 on 8 %.  Two more
  data sets pin the rounding: "wide" (w2 in {0, 1} at density 1/2, t1 in halves of [0, 8], 5 pixels: y2 beyond 256 in halves -- ties and non-ties -- with exact
  statistics of the UNROUNDED y2) and "fine" (t1 in 128ths: h1 and y2 beyond 8 bits; no statistics).

Every output is pre-filled with SENTINEL, spare rows included, and is a channel slice of a wider buffer where the C ABI takes a
pitch; partial-row buffers are NaN-filled and workspaces filled with 0xFF bytes (NaN as fp32 and as fp64); the channels beside a
pitched / sliced input hold GARBAGE.

Form -> case:

* ``meta_relative_kernel`` ...................................... test_relative (random fp32 cart, every image; fp16 build)
* ``meta_modulate_kernel`` (lanes 256/(C/8): 32 .. 1; 252 / 240 / 240 active threads at C = 24 / 96 / 160) ... test_gathers[*],
  grid-stride beyond the 4096-workgroup cap test_gathers_beyond_grid_cap, fp16 build test_modulate_fp16_build
* ``meta_modulate_bwd_pos_kernel`` + ``_bwd_feat_kernel`` ........ test_gathers[*], test_gathers_beyond_grid_cap
* ``meta_bwd_sums_kernel`` (one 512-pixel row per workgroup) ..... test_gathers[*]; two rows, the second ragged: [1x9x61-*]
* ``meta_bwd_apply_kernel`` ..................................... test_gathers[*], test_gathers_beyond_grid_cap
* ``smallk_moments_kernel<4|8>`` ................................ test_smallk[cin<=4|cin>=5]; 1023 / 1024 blocks test_smallk_moment_blocks
* ``smallk_stats_kernel<4|8>`` (host and device count) .......... test_smallk[*] (training form)
* ``smallk_apply_kernel<4|8>`` .................................. test_smallk[*]; grid cap test_smallk_forward_beyond_grid_cap; fp16 build
  test_smallk_forward_fp16_build
* ``bn_bwd_smallk_reduce_kernel<4|8, true>`` (flags 5 and 4), ``<4|8, false>`` (stored y, with and without the mask) ... test_smallk[*]
* ``bn_bwd_smallk_finalize_kernel<4|8>`` (one call, two calls, SyncBN) ... test_smallk[*]
* ``pos_fwd_kernel<256|128, false>`` ............................ test_pos_forward[*] (idle workgroups: every C = 128 case with an odd
  step count, and P = 1), test_pos_forward_rounding
* ``pos_fwd_kernel<256|128, true>`` ............................. test_pos_modulate_forward[*]
* ``pos_bwd_kernel<256|128>`` ................................... test_pos_backward_sums[*] (several steps per workgroup: 129, 300, 999, ...)

test_argument_checks pins the rejections.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import bn_ref as R
import stem_ref as S
from test_gpu_bn_passes import GARBAGE, SENTINEL, SPARE, _check_partial, _L
from test_gpu_forward import DEV

pytestmark = pytest.mark.gpu

LAYOUTS = ("dense", "pitched", "offset")
BF16, F16 = torch.bfloat16, torch.float16
U24 = float(1 << 24)


# ------------------------------------------------------------------------------------------------------------------ helpers
class _Gen:
    """Small-integer data from a seeded CPU generator (the same numbers wherever the test runs), moved to the device as fp32."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def ints(self, lo, hi, shape, step=1.0):
        return (torch.randint(lo, hi + 1, shape, generator=self.g).float() * step).to(DEV)

    def pick(self, values, shape):
        return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=self.g)].to(DEV)

    def rand(self, shape, lo=0.0, hi=1.0):
        return (lo + (hi - lo) * torch.rand(shape, generator=self.g)).to(DEV)

    def sparse(self, shape, density_inv):
        """{-1, 0, 1} with a non-zero every `density_inv` elements on average."""
        keep = torch.randint(0, density_inv, shape, generator=self.g) == 0
        return ((torch.randint(0, 2, shape, generator=self.g) * 2 - 1) * keep).float().to(DEV)


def _place(t, layout, width=None):
    """(view, row pitch) of an INPUT in a layout: dense; pitched (ld = C + 8); offset: the upper slice of a 2C-wide buffer.  The
    channels beside it hold GARBAGE."""
    rows, c = t.shape
    if layout == "dense":
        return t.contiguous(), c
    ld, off = (c + 8, 0) if layout == "pitched" else (2 * c, c)
    buf = torch.full((rows, ld), GARBAGE, dtype=t.dtype, device=DEV)
    buf[:, off:off + c] = t
    return buf[:, off:off + c], ld


class _Out:
    """An OUTPUT of `rows` x c: SENTINEL-filled with SPARE rows behind; in the pitched / offset layouts a channel slice of a wider buffer."""

    def __init__(self, rows, c, dtype, layout="dense"):
        self.rows, self.c = rows, c
        self.ld, self.off = {"dense": (c, 0), "pitched": (c + 8, 0), "offset": (2 * c, c)}[layout]
        self.buf = torch.full((rows + SPARE, self.ld), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[:rows, self.off:self.off + c]

    def untouched_outside(self, what):
        b = self.buf
        ok = bool((b[self.rows:] == SENTINEL).all()) and bool((b[:, :self.off] == SENTINEL).all()) and bool((b[:, self.off + self.c:] == SENTINEL).all())
        assert ok, f"{what}: wrote outside its slice"

    def untouched(self, what):
        assert bool((self.buf == SENTINEL).all()), f"{what}: the rejected call wrote"

    def check(self, ref, what):
        _eq(self.view, ref, what)
        self.untouched_outside(what)


def _fits_fp32(ref, what):
    assert torch.equal(ref.float().double(), ref), f"{what}: the exact result does not fit fp32 (data rule)"


def _eq(got, ref, what):
    """got (storage type) equals the exact fp64 `ref` rounded once, bit for bit."""
    _fits_fp32(ref, what)
    ref_s = ref.to(got.dtype)
    if torch.equal(got, ref_s):
        return
    bad = (got != ref_s) | got.isnan()
    px, ch = bad.nonzero(as_tuple=True)
    first = [(int(p), int(c), float(got[p, c]), float(ref_s[p, c]), float(ref[p, c])) for p, c in zip(px[:6].tolist(), ch[:6].tolist())]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; rows {int(px.min())}..{int(px.max())}, "
                         f"channels {sorted(set(ch.tolist()))[:16]}; first (row, channel, got, want, exact): {first}")


def _rounds(ref, dtype):
    """(some element is not representable, some element is an exact tie) of the exact fp64 values (which fit fp32, and are fp16-normal)
    in the storage type: the fp32 significand bits the storage type drops -- 16 for bf16, 13 for fp16."""
    drop = 16 if dtype == BF16 else 13
    low = ref.float().contiguous().view(torch.int32) & ((1 << drop) - 1)
    return bool((low != 0).any()), bool((low == (1 << (drop - 1))).any())


def _row_sums_exact(term_absmax, terms_per_row, unit, what):
    """The precondition of an exact fp32 partial row: every partial sum is a count of `unit`s below 2^24."""
    assert float(term_absmax) * terms_per_row / unit < U24, f"{what}: {float(term_absmax)} x {terms_per_row} / {unit} reaches 2^24 (data rule)"


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _ff_bytes(n):
    """A workspace of n bytes, every byte 0xFF: NaN whether a kernel reads it as fp32 or as fp64."""
    return torch.full((int(n) + 8,), 255, dtype=torch.uint8, device=DEV)


def _sync():
    torch.cuda.synchronize()


def _call(dtype, name, *args):
    L = _L()
    if dtype == F16:
        with L.operand("f16"):
            L.call(name, *args)
    else:
        L.call(name, *args)


# ================================================================================================================== gathers
class _Gather:
    """The operands of one (N, H, W, C) case in the storage type; `fine`: feat in eighths, dgeo and shift in quarters (every element-wise output rounds; the sums would not be exact)."""

    def __init__(self, dims, c, seed, dtype=BF16, fine=False):
        g = _Gen(seed)
        n, h, w = dims
        self.dims, self.c, self.dtype, self.px = dims, c, dtype, n * h * w
        px = self.px
        self.pos = g.ints(-6, 6, (px * 9, c)).to(dtype)
        self.feat = (g.ints(-63, 63, (px, c), 0.125) if fine else g.ints(-4, 4, (px, c))).to(dtype)
        self.dgeo = (g.ints(-31, 31, (px, 9 * c), 0.25) if fine else g.ints(-3, 3, (px, 9 * c))).to(dtype)
        self.scale, self.shift = g.pick([-1.0, 0.5, 1.0, 2.0], (c,)), (g.ints(-16, 16, (c,), 0.25) if fine else g.ints(-4, 4, (c,)))
        self.mean, self.invstd = g.ints(-4, 4, (c,), 0.5), g.pick([0.5, 1.0, 2.0], (c,))
        self.coef = torch.stack([g.pick([-2.0, -0.5, 0.5, 1.0, 2.0], (c,)), g.ints(-2, 2, (c,)), g.pick([-1.0, -0.5, 0.0, 0.5, 1.0], (c,))]).contiguous()
        self.inside = S.gather9(torch.ones(px, 1, dtype=torch.float64, device=DEV), dims) > 0  # (px, 9, 1)


def _ptrs(*ts):
    L = _L()
    return [L.ptr(t) for t in ts]


def _run_modulate(D, layout, what):
    L = _L()
    n, h, w = D.dims
    feat, ld_feat = _place(D.feat, layout)
    geo = _Out(D.px, 9 * D.c, D.dtype)
    ref = S.modulate(D.pos, D.scale, D.shift, D.feat, D.dims)
    _fits_fp32(ref, what)
    _call(D.dtype, "rv_meta_modulate", *_ptrs(D.pos, D.scale, D.shift, feat), ld_feat, n, h, w, D.c, L.ptr(geo.view), L.stream_ptr())
    _sync()
    geo.check(ref, what + " geo")
    border = ~D.inside.expand(D.px, 9, D.c).reshape(D.px, 9 * D.c)
    assert bool((geo.view[border] == 0).all()), what + ": a tap outside the image is not exactly 0"
    return ref


def _run_bwd(D, layout, what):
    L = _L()
    n, h, w = D.dims
    feat, ld_feat = _place(D.feat, layout)
    dpos, dfeat = _Out(D.px * 9, D.c, D.dtype), _Out(D.px, D.c, D.dtype, layout)
    ref_dpos, ref_dfeat = S.modulate_bwd(D.dgeo, D.pos, D.scale, D.shift, D.feat, D.dims)
    _fits_fp32(ref_dpos, what), _fits_fp32(ref_dfeat, what)
    _call(D.dtype, "rv_meta_modulate_bwd", *_ptrs(D.dgeo, D.pos, D.scale, D.shift, feat), ld_feat, n, h, w, D.c,
          L.ptr(dpos.view), L.ptr(dfeat.view), dfeat.ld, L.stream_ptr())
    _sync()
    dpos.check(ref_dpos, what + " dpos_act")
    dfeat.check(ref_dfeat, what + " dfeat")
    return ref_dpos, ref_dfeat


def _run_bwd_sums(D, layout, what, sums_exact=True):
    L = _L()
    n, h, w = D.dims
    feat, ld_feat = _place(D.feat, layout)
    rows = L.load().rv_meta_bwd_rows(n, h, w)
    assert rows == (D.px + 511) // 512
    z = S.modulate_z(D.dgeo, D.pos, D.scale, D.shift, D.feat, D.dims)
    xh = R.xhat(D.pos, D.mean, D.invstd)
    if sums_exact:
        _row_sums_exact((z * xh).abs().max(), min(D.px, 512) * 9, 0.25, what)
    s0, s1, ref_dfeat = S.modulate_bwd_sums(D.dgeo, D.pos, D.scale, D.shift, D.mean, D.invstd, D.feat, D.dims)
    _fits_fp32(ref_dfeat, what)
    # the strict gate: some gate sits exactly on 0 where the gradient and the feature are not 0, and a border tap carries a gradient
    live = (D.dgeo.double().reshape(-1, D.c) != 0) & (S.gather9(D.feat.double(), D.dims).reshape(-1, D.c) != 0)
    on_zero = (D.pos.double() * D.scale.double() + D.shift.double()) == 0
    if sums_exact and D.px * D.c >= 256:
        assert bool((on_zero & live).any()), what + ": no gate exactly on 0 (data)"
    dfeat = _Out(D.px, D.c, D.dtype, layout)
    partial = _nan(rows + L.STATS_SCRATCH_ROWS, 2, D.c)
    _call(D.dtype, "rv_meta_modulate_bwd_sums", *_ptrs(D.dgeo, D.pos, D.scale, D.shift, D.mean, D.invstd, feat), ld_feat, n, h, w,
          D.c, L.ptr(dfeat.view), dfeat.ld, L.ptr(partial), L.stream_ptr())
    _sync()
    dfeat.check(ref_dfeat, what + " dfeat (fused)")
    if sums_exact:
        _check_partial(partial, rows, s0, s1, what + " partial")
    else:  # (the fine data: written, no more)
        assert bool(torch.isfinite(partial[:rows]).all()) and bool(partial[rows:].isnan().all()), what + ": partial rows"
    return ref_dfeat


def _run_bwd_apply(D, layout, what):
    L = _L()
    n, h, w = D.dims
    feat, ld_feat = _place(D.feat, layout)
    dy = _Out(D.px * 9, D.c, D.dtype)
    ref = S.modulate_bwd_apply(D.dgeo, D.pos, D.scale, D.shift, D.mean, D.invstd, D.coef, D.feat, D.dims)
    _fits_fp32(ref, what)
    _call(D.dtype, "rv_meta_modulate_bwd_apply", *_ptrs(D.dgeo, D.pos, D.scale, D.shift, D.mean, D.invstd, D.coef, feat), ld_feat, n, h,
          w, D.c, L.ptr(dy.view), L.stream_ptr())
    _sync()
    dy.check(ref, what + " dy")
    # a tap outside the image: dy = coef0 (0 - coef1 - xhat coef2), spelled out
    border = ~D.inside.reshape(-1)
    k = D.coef.double()
    want = (k[0] * (0.0 - k[1] - R.xhat(D.pos, D.mean, D.invstd) * k[2]))[border]
    assert torch.equal(dy.view[border], want.to(D.dtype)), what + ": dy of a tap outside the image"
    return ref


IMAGES = [(1, 1, 1), (1, 1, 5), (2, 3, 7), (1, 4, 8), (2, 5, 37), (3, 2, 65), (1, 9, 61)]  # the last: 549 pixels, two partial rows
GATHER_C = [8, 24, 96, 160, 256]
GATHER_CASES = [(d, c, LAYOUTS[(i + j) % 3]) for i, d in enumerate(IMAGES) for j, c in enumerate(GATHER_C)] + \
               [(d, 2048, LAYOUTS[i]) for i, d in enumerate(IMAGES[:3])]


def _gid(case):
    (n, h, w), c, layout = case
    return f"{n}x{h}x{w}-{c}-{layout}"


@pytest.mark.parametrize("case", GATHER_CASES, ids=_gid)
def test_gathers(case):
    """rv_meta_modulate, _bwd, _bwd_sums and _bwd_apply on one image: every output bit for bit, the partial rows exactly."""
    dims, c, layout = case
    D = _Gather(dims, c, seed=dims[2] * 10000 + c)
    what = f"{_gid(case)}"
    ref_geo = _run_modulate(D, layout, what)
    _run_bwd(D, layout, what)
    _run_bwd_sums(D, layout, what)
    _run_bwd_apply(D, layout, what)
    assert _rounds(ref_geo, D.dtype) == (False, False)
    # the fine data: every element-wise output goes beyond 8 significant bits, ties included (the sums are then not exact: not compared)
    F = _Gather(dims, c, seed=dims[2] * 10000 + c + 1, fine=True)
    what += " fine"
    refs = [_run_modulate(F, layout, what), *_run_bwd(F, layout, what), _run_bwd_sums(F, layout, what, sums_exact=False), _run_bwd_apply(F, layout, what)]
    if D.px * c >= 4096:
        assert all(_rounds(r, D.dtype) == (True, True) for r in refs), what + ": no rounding case (data)"


def test_gathers_beyond_grid_cap():
    """1 x 8 x 512 x 256: 4608 workgroups' worth of items against grid_for's cap of 4096 -- the grid-stride rounds of rv_meta_modulate,
    _bwd and _bwd_apply."""
    dims, c = (1, 8, 512), 256
    assert dims[0] * dims[1] * dims[2] * 9 * (c // 8) > 4096 * 256
    D = _Gather(dims, c, seed=4096)
    _run_modulate(D, "dense", "cap")
    _run_bwd(D, "pitched", "cap")
    _run_bwd_apply(D, "offset", "cap")


@pytest.mark.parametrize("case", [((2, 5, 37), 96, "pitched"), ((3, 2, 65), 256, "offset"), ((1, 1, 5), 8, "dense")], ids=_gid)
def test_modulate_fp16_build(case):
    """rv_meta_modulate of the fp16-operand build on the same data (the fine data round in fp16 too: 13 bits against 11)."""
    dims, c, layout = case
    for fine in (False, True):
        D = _Gather(dims, c, seed=dims[2] * 10000 + c + fine, dtype=F16, fine=fine)
        ref = _run_modulate(D, layout, f"{_gid(case)} fp16 fine={fine}")
    if dims[2] > 5:
        assert _rounds(ref, F16) == (True, True)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dims", IMAGES, ids=lambda d: "x".join(map(str, d)))
def test_relative(dims, dtype):
    """rv_meta_relative on RANDOM fp32 cart: one fp32 subtraction and one rounding -- bit-exact by construction.  Channels 3..31 zero."""
    L = _L()
    n, h, w = dims
    g = _Gen(n * 100 + w)
    cart = (g.rand((n, 3, h, w), -1.0, 1.0) * g.pick([0.01, 1.0, 80.0, 2.0e4 if dtype == F16 else 3.0e4], (n, 3, h, w))).contiguous()
    assert float(cart.abs().max()) * 2 < 6.0e4
    ref = S.relative(cart, dtype)
    rel = _Out(n * h * w * 9, 32, dtype)
    _call(dtype, "rv_meta_relative", L.ptr(cart), n, h, w, L.ptr(rel.view), L.stream_ptr())
    _sync()
    rel.check(ref, f"relative {dims} {dtype}")
    if n * h * w > 1:
        c = cart.permute(0, 2, 3, 1).reshape(-1, 3)
        assert _rounds((S.gather9(c, dims) - c[:, None]).double(), dtype)[0]


# ================================================================================================================== small-K layers
SMALLK_PIXELS = [1, 511, 512, 513, 1500]


class _SmallK:
    def __init__(self, n, c, cin, seed, dtype=BF16, garbage=True):
        g = _Gen(seed)
        self.n, self.c, self.cin, self.dtype = n, c, cin, dtype
        self.cin_pad = 4 if cin <= 4 else 8
        v = torch.full((n, 32), GARBAGE if garbage else 0.0, dtype=torch.float32, device=DEV)
        v[:, :cin] = g.ints(-3, 3, (n, cin))
        self.v32 = v.to(dtype)                      # ld_v = 32
        self.v8 = self.v32[:, :8].contiguous()      # ld_v = 8
        w = torch.full((c, 8), GARBAGE, dtype=torch.float32, device=DEV)
        w[:, :cin] = g.ints(-1, 1, (c, cin))
        w[:, 0] = g.pick([-1.0, 1.0], (c,))          # no all-zero row: var(y) >= 1
        self.w_garbage = w.to(dtype)                # for the launches that read no column at or beyond cin
        w = w.clone()
        w[:, cin:self.cin_pad] = 0.0                # zero weight columns against the garbage channels of v (include/rv3d.h)
        self.w = w.to(dtype)
        act = lambda lo, hi: g.ints(lo, hi, (n, c)).to(dtype)
        self.dout, self.out, self.y = act(-4, 4), act(-2, 2), act(-6, 6)
        self.scale, self.shift = g.pick([-1.0, 0.5, 1.0, 2.0], (c,)), g.ints(-4, 4, (c,), 0.5)
        self.shift_fine = g.ints(-255, 255, (c,), 1.0 / 64)
        self.mean, self.invstd = g.ints(-4, 4, (c,), 0.5), g.pick([0.5, 1.0, 2.0], (c,))
        self.gamma, self.beta = g.rand((c,), 0.5, 1.5), g.rand((c,), -1.0, 1.0)
        self.rmean, self.rvar = g.rand((c,), -1.0, 1.0), g.rand((c,), 0.5, 2.0)

    def vin(self, ld_v, n):
        return (self.v8 if ld_v == 8 else self.v32)[:n], ld_v


_smallk_cache = {}


def _smallk(c, cin):
    if (c, cin) not in _smallk_cache:
        _smallk_cache[(c, cin)] = _SmallK(1500, c, cin, seed=c * 10 + cin)
    return _smallk_cache[(c, cin)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _smallk_cache.clear()
    _pos_cache.clear()
    torch.cuda.empty_cache()


EPS = float(torch.tensor(1e-5, dtype=torch.float32))
MOM = float(torch.tensor(0.1, dtype=torch.float32))


def _moments(D, v, ld_v, n, what, extra=0):
    """rv_smallk_moments into a NaN-filled buffer (+ `extra` doubles behind); == the reference."""
    L = _L()
    lib = L.load()
    cols = D.cin_pad + D.cin_pad ** 2
    m1, m2 = S.smallk_moments(v, D.cin_pad)
    _row_sums_exact(float(v[:, :D.cin_pad].abs().max()) ** 2, 257, 1.0, what)  # a moment block covers ceil(n / blocks) <= 257 pixels
    ws = _ff_bytes(lib.rv_smallk_forward_workspace_bytes(D.cin))
    mom = _nan(cols + extra, dtype=torch.float64)
    L.call("rv_smallk_moments", L.ptr(v), ld_v, n, D.cin, L.ptr(mom), L.ptr(ws), L.stream_ptr())
    _sync()
    want = torch.cat([m1, m2.reshape(-1)])
    assert torch.equal(mom[:cols], want), f"{what}: moments differ at {(mom[:cols] != want).nonzero().flatten().tolist()[:8]}"
    assert bool(mom[cols:].isnan().all())
    return mom


def _forward(D, v, ld_v, n, w, scale, shift, relu, layout, dtype=BF16, moments=None, count=0, stats=None, want_h=True):
    """rv_smallk_forward.  Eval form: moments None.  Training: `stats` = dict of output tensors (scale, shift, mean, invstd, rmean, rvar)."""
    L = _L()
    h = _Out(n, D.c, dtype, layout) if want_h else None
    st = stats or {}
    _call(dtype, "rv_smallk_forward", L.ptr(v), ld_v, n, D.cin, L.ptr(w), 8, D.c, L.ptr(moments), count,
          L.ptr(D.gamma if moments is not None else None), L.ptr(D.beta if moments is not None else None), EPS, MOM, L.ptr(st.get("rmean")),
          L.ptr(st.get("rvar")), L.ptr(scale), L.ptr(shift), L.ptr(st.get("mean")), L.ptr(st.get("invstd")), 1 if relu else 0,
          L.ptr(h.view) if h else None, h.ld if h else D.c, L.stream_ptr())
    _sync()
    return h


def _stat_outputs(D):
    return {"scale": _nan(D.c), "shift": _nan(D.c), "mean": _nan(D.c), "invstd": _nan(D.c), "rmean": D.rmean.clone(), "rvar": D.rvar.clone()}


def _within(got, ref, abs_terms, what):
    """|got - ref| <= 2^-23 x the sum of the absolute terms: fp64 arithmetic on exact moments, then one cast to fp32."""
    err = (got.double() - ref).abs()
    bound = 2.0 ** -23 * abs_terms
    assert bool((err <= bound).all()), f"{what}: {float((err / bound.clamp_min(1e-300)).max()):.2f} x the bound at channel {int((err / bound.clamp_min(1e-300)).argmax())}"


def _check_training(D, v, ld_v, n, layout, what):
    mom = _moments(D, v, ld_v, n, what, extra=1)
    cols = D.cin_pad + D.cin_pad ** 2
    ref = S.smallk_stats(v, D.w, D.cin, D.gamma, D.beta, EPS, MOM, D.rmean, D.rvar)
    st = _stat_outputs(D)
    h = _forward(D, v, ld_v, n, D.w, st["scale"], st["shift"], True, layout, moments=mom, count=n, stats=st)
    if n >= 500:  # var >= 1: the closed form's cancellation stays at 1e-14
        assert float(S.smallk_y(v, D.w, D.cin).var(0, unbiased=False).min()) >= 1.0
    mean_sc = (ref["mean"] * ref["scale"]).abs()
    _within(st["scale"], ref["scale"], ref["scale"].abs(), what + " scale")
    _within(st["shift"], ref["shift"], D.beta.double().abs() + mean_sc, what + " shift")
    _within(st["mean"], ref["mean"], ref["mean"].abs(), what + " mean")
    _within(st["invstd"], ref["invstd"], ref["invstd"].abs(), what + " invstd")
    _within(st["rmean"], ref["running_mean"], ((1 - MOM) * D.rmean.double()).abs() + (MOM * ref["mean"]).abs(), what + " running_mean")
    _within(st["rvar"], ref["running_var"], ref["running_var"].abs(), what + " running_var")
    # h equals the eval-form launch fed the kernel's own scale / shift, bit for bit
    h_eval = _forward(D, v, ld_v, n, D.w, st["scale"], st["shift"], True, layout)
    assert torch.equal(h.view, h_eval.view), what + ": training-form h differs from the eval form on the same scale / shift"
    h.untouched_outside(what + " h")
    # h = NULL: the statistics and nothing else; neither the weight columns nor the moments of the channels at and beyond cin are read
    # (GARBAGE in the former, NaN in the latter)
    unused = torch.ones(D.cin_pad, dtype=torch.bool, device=DEV)
    unused[:D.cin] = False
    mom_nan = mom.clone()
    mom_nan[:cols][torch.cat([unused, (unused[:, None] | unused[None, :]).reshape(-1)])] = float("nan")
    st2 = _stat_outputs(D)
    _forward(D, v, ld_v, n, D.w_garbage, st2["scale"], st2["shift"], True, layout, moments=mom_nan, count=n, stats=st2, want_h=False)
    # count < 0: the count is the double behind the moments
    mom[-1] = float(n)
    st3 = _stat_outputs(D)
    h3 = _forward(D, v, ld_v, n, D.w, st3["scale"], st3["shift"], True, layout, moments=mom, count=-1, stats=st3)
    for k in st:
        assert torch.equal(st[k], st2[k]), f"{what}: {k} of the statistics-only launch differs"
        assert torch.equal(st[k], st3[k]), f"{what}: {k} with the device-side count differs"
    assert torch.equal(h.view, h3.view)
    return st


def _sums(D, n, ld_v, layout, flags, use_out, what):
    """rv_bn_bwd_smallk_sums: sums[0 : (2 + cin) c] and moms == the reference."""
    L = _L()
    lib = L.load()
    v, _ = D.vin(ld_v, n)
    recomp = bool(flags & S.BNB_Y_FROM_INPUT)
    (dout, ld_dout), (out, ld_out), (y, ld_y) = _place(D.dout[:n], layout), _place(D.out[:n], layout), _place(D.y[:n], layout)
    s0, s1, r, g = S.smallk_bwd_planes(D.dout[:n], D.out[:n] if use_out else None, D.y[:n], v, D.w, D.cin, D.cin_pad, D.scale, D.shift, D.mean, D.invstd, flags)
    yy = S.smallk_y(v, D.w, D.cin) if recomp else D.y[:n].double()
    xh = R.xhat(yy, D.mean, D.invstd)
    _row_sums_exact((g * xh).abs().max(), 512, 0.25, what)
    _row_sums_exact(float(g.abs().max()) * float(v[:, :D.cin_pad].abs().max()), 512, 1.0, what)
    assert rows_of(n) == (n + 511) // 512
    planes, cols = 2 + D.cin_pad, D.cin_pad + D.cin_pad ** 2
    ws = _ff_bytes(lib.rv_bn_bwd_smallk_workspace_bytes(n, D.c, D.cin))
    sums, moms = _nan(planes * D.c, dtype=torch.float64), _nan(cols, dtype=torch.float64)
    L.call("rv_bn_bwd_smallk_sums", n, D.c, L.ptr(dout), ld_dout, L.ptr(out) if use_out else None, ld_out if use_out else 0,
           L.ptr(None if recomp else y), 0 if recomp else ld_y, *_ptrs(D.scale, D.shift, D.mean, D.invstd), flags, L.ptr(v), ld_v, D.cin,
           L.ptr(D.w if recomp else None), 8, L.ptr(sums), L.ptr(moms), L.ptr(ws), L.stream_ptr())
    _sync()
    want = torch.cat([s0, s1, r[:D.cin].reshape(-1)])
    got = sums[: (2 + D.cin) * D.c]
    assert torch.equal(got, want), f"{what}: sums differ in planes {sorted(set(((got != want).nonzero().flatten() // D.c).tolist()))}"
    m1, m2 = S.smallk_moments(v, D.cin_pad)
    assert torch.equal(moms, torch.cat([m1, m2.reshape(-1)])), what + ": moms differ"
    return sums, moms, (s0, s1, r, g, yy, xh)


def rows_of(n):
    L = _L()
    return L.load().rv_bn_bwd_rows(n)


def _grads(D, n, ld_v, what):
    """rv_bn_bwd_smallk_from_sums, the one-call rv_bn_bwd_smallk and the SyncBN form."""
    L = _L()
    lib = L.load()
    flags = S.BNB_Y_FROM_INPUT | S.BNB_RELU_Z
    v, _ = D.vin(ld_v, n)
    sums, moms, (s0, s1, r, g, yy, xh) = _sums(D, n, ld_v, "dense", flags, False, what)
    vd = v[:, :D.cin].double()

    def check(dg, db, dw, global_s01, count, tag):
        ref_dg, ref_db, ref_dw = S.smallk_grads(g, yy, v, D.cin, D.gamma, D.mean, D.invstd, global_s01, count)
        assert torch.equal(dg, ref_dg.float()) and torch.equal(db, ref_db.float()), f"{what} {tag}: dgamma / dbeta"
        k0 = (D.gamma.double() * D.invstd.double()).abs()[:, None]
        t0, t1 = (s0, s1) if global_s01 is None else (global_s01[0], global_s01[1])
        k1, k2 = (t0 / count).abs()[:, None], (t1 / count).abs()[:, None]
        terms = k0 * (r[:D.cin].t().abs() + k1 * vd.sum(0).abs()[None] + k2 * (xh.t() @ vd).abs())
        _within(dw, ref_dw, terms, f"{what} {tag} dW")

    def outputs():
        return torch.full((D.c,), SENTINEL, device=DEV), torch.full((D.c,), SENTINEL, device=DEV), torch.full((D.c + 1, D.cin), SENTINEL, device=DEV)

    dg, db, dw = outputs()
    L.call("rv_bn_bwd_smallk_from_sums", D.c, D.cin, L.ptr(sums), L.ptr(moms), None, L.ptr(D.w_garbage), 8, *_ptrs(D.gamma, D.mean, D.invstd),
           n, L.ptr(dg), L.ptr(db), L.ptr(dw), L.stream_ptr())
    _sync()
    check(dg, db, dw[:D.c], None, n, "two calls")
    assert bool((dw[D.c:] == SENTINEL).all())
    # one call
    ws = _ff_bytes(lib.rv_bn_bwd_smallk_workspace_bytes(n, D.c, D.cin))
    dg1, db1, dw1 = outputs()
    L.call("rv_bn_bwd_smallk", n, D.c, L.ptr(D.dout[:n]), D.c, None, 0, None, 0, *_ptrs(D.scale, D.shift, D.mean, D.invstd),
           flags, L.ptr(v), ld_v, D.cin, L.ptr(D.w), 8, L.ptr(D.gamma), None, None, n, L.ptr(dg1), L.ptr(db1), L.ptr(dw1), L.ptr(ws),
           L.stream_ptr())
    _sync()
    assert torch.equal(dg1, dg) and torch.equal(db1, db) and torch.equal(dw1, dw), what + ": the one-call form differs from the two-call form"
    # SyncBN: global sums = twice the local ones, the count 2 n read from the device
    gs = torch.cat([2 * s0, 2 * s1, torch.tensor([2.0 * n], dtype=torch.float64, device=DEV)])
    dg2, db2, dw2 = outputs()
    L.call("rv_bn_bwd_smallk_from_sums", D.c, D.cin, L.ptr(sums), L.ptr(moms), L.ptr(gs), L.ptr(D.w), 8, *_ptrs(D.gamma, D.mean, D.invstd),
           -1, L.ptr(dg2), L.ptr(db2), L.ptr(dw2), L.stream_ptr())
    _sync()
    check(dg2, db2, dw2[:D.c], torch.stack([2 * s0, 2 * s1]), 2 * n, "SyncBN")


SMALLK_CASES = [(cin, c) for cin in (1, 2, 3, 4, 5, 6, 8) for c in (8, 64, 96, 256)]


@pytest.mark.parametrize("cin,c", SMALLK_CASES, ids=[f"cin{a}-c{b}" for a, b in SMALLK_CASES])
def test_smallk(cin, c):
    """Every small-K entry point at one (cin, c), pixels 1 / 511 / 512 / 513 / 1500, ld_v 8 and 32, the three layouts."""
    D = _smallk(c, cin)
    for i, n in enumerate(SMALLK_PIXELS):
        ld_v = (8, 32)[(i + cin) % 2]
        layout = LAYOUTS[(i + cin + c // 8) % 3]
        what = f"smallk cin={cin} c={c} n={n} ld_v={ld_v} {layout}"
        v, _ = D.vin(ld_v, n)
        _moments(D, v, ld_v, n, what)
        # eval form: power-of-two scale, shift in halves (exact) and in 64ths (rounds)
        for relu in (True, False):
            h = _forward(D, v, ld_v, n, D.w, D.scale, D.shift, relu, layout)
            h.check(S.smallk_apply(v, D.w, cin, D.scale, D.shift, relu), f"{what} eval relu={relu}")
        ref = S.smallk_apply(v, D.w, cin, D.scale, D.shift_fine, False)
        _forward(D, v, ld_v, n, D.w, D.scale, D.shift_fine, False, layout).check(ref, what + " eval fine")
        if n * c >= 4096:
            assert _rounds(ref, BF16) == (True, True), what + ": no rounding case (data)"
        _check_training(D, v, ld_v, n, layout, what)
        _sums(D, n, ld_v, layout, S.BNB_Y_FROM_INPUT | S.BNB_RELU_Z, False, what + " recompute+relu_z")
        _sums(D, n, ld_v, layout, S.BNB_Y_FROM_INPUT, False, what + " recompute")
        _sums(D, n, ld_v, layout, S.BNB_Y_FROM_INPUT | S.BNB_RELU_Z, True, what + " recompute+relu_z+mask")
        _sums(D, n, ld_v, layout, S.BNB_RELU_Z, False, what + " stored y+relu_z")
        _sums(D, n, ld_v, layout, 0, True, what + " stored y+mask")
        _grads(D, n, ld_v, what)
    assert bool((D.out == 0).any())
    recomputed_on_zero = (S.smallk_y(D.v8, D.w, cin) * D.scale.double() + D.shift.double()) == 0
    assert bool(recomputed_on_zero.any()) or c * cin < 64, "no recomputed gate exactly on 0 (data)"


@pytest.mark.parametrize("n", [262143, 262144])
def test_smallk_moment_blocks(n):
    """The moment-block switch at 262 144 pixels (c = 64, cin = 3): ceil(n / 256) blocks below it, 1024 blocks from it on."""
    D = _SmallK(n, 64, 3, seed=n)
    v, ld_v = D.vin(8, n)
    _moments(D, v, ld_v, n, f"moments n={n}")
    _sums(D, n, 8, "dense", S.BNB_Y_FROM_INPUT | S.BNB_RELU_Z, False, f"sums n={n}")


def test_smallk_forward_beyond_grid_cap():
    """c = 256 (8 pixel lanes): 40 000 pixels are 5000 workgroups' worth against the cap of 4096 -- ranges of more than one round."""
    D = _SmallK(40000, 256, 3, seed=40000)
    assert (40000 + 7) // 8 > 4096
    v, ld_v = D.vin(32, D.n)
    _forward(D, v, ld_v, D.n, D.w, D.scale, D.shift_fine, True, "pitched").check(S.smallk_apply(v, D.w, 3, D.scale, D.shift_fine, True), "grid cap")


@pytest.mark.parametrize("cin,c", [(3, 64), (5, 96), (8, 256)])
def test_smallk_forward_fp16_build(cin, c):
    D = _SmallK(513, c, cin, seed=c + cin, dtype=F16)
    v, ld_v = D.vin(8, D.n)
    for relu, shift in ((True, D.shift), (False, D.shift_fine)):
        _forward(D, v, ld_v, D.n, D.w, D.scale, shift, relu, "offset", dtype=F16).check(S.smallk_apply(v, D.w, cin, D.scale, shift, relu), f"fp16 cin={cin} c={c} relu={relu}")


# ================================================================================================================== positional pair
class _Pos:
    """The operands of one (P, C, cin) case.  kind: "base" (the recipe), "wide" (w2 in {0, 1} at density 1/2, t1 in [0, 8]), "fine" (t1 in 128ths)."""

    def __init__(self, p, c, cin, seed, dtype=BF16, kind="base"):
        g = _Gen(seed)
        self.p, self.c, self.cin, self.dtype = p, c, cin, dtype
        rel = torch.full((p, 32), GARBAGE, dtype=torch.float32, device=DEV)
        rel[:, :cin] = g.ints(-3, 3, (p, cin))
        self.rel32 = rel.to(dtype)
        w1 = torch.full((c, 8), GARBAGE, dtype=torch.float32, device=DEV)  # (the pair reads the columns below cin only)
        w1[:, :cin] = g.ints(-1, 1, (c, cin))
        self.w1 = w1.to(dtype)
        self.s1 = g.pick([0.5, 1.0], (c,))
        self.t1 = g.ints(-255, 255, (c,), 1.0 / 128) if kind == "fine" else (g.ints(0, 16, (c,), 0.5) if kind == "wide" else g.ints(-4, 4, (c,), 0.5))
        self.w2 = (g.sparse((c, c), 2).abs() if kind == "wide" else g.sparse((c, c), 8)).to(dtype)
        self.w2s = self.w2.t().contiguous()
        self.dy2 = g.ints(-2, 2, (p, c)).to(dtype)
        self.mean1, self.invstd1 = g.ints(-4, 4, (c,), 0.5), g.pick([0.5, 1.0, 2.0], (c,))
        self.s2, self.t2 = g.pick([-1.0, 0.5, 1.0, 2.0], (c,)), g.ints(-8, 8, (c,), 0.5)

    def rel(self, ld):
        """rel with row pitch 4, 8 or 32 (channels cin.. hold GARBAGE)."""
        return (self.rel32 if ld == 32 else self.rel32[:, :ld].contiguous()), ld


_pos_cache = {}


def _pos(c, dtype=BF16):
    """The big case of a channel count (one persistent round plus one pixel), shared: smaller P are its leading pixels."""
    if (c, dtype) not in _pos_cache:
        _pos_cache[(c, dtype)] = _Pos(256 * (128 * 256 // c) + 1, c, 3, seed=c + (dtype == F16), dtype=dtype)
    return _pos_cache[(c, dtype)]


def _run_pos_forward(D, p, cin, ld_rel, with_stats, what, kind="base"):
    L = _L()
    c, dtype = D.c, D.dtype
    rel, _ = D.rel(ld_rel)
    rel = rel[:p]
    w1 = D.w1
    if cin != D.cin:  # fewer input channels of the same data: the weight columns at and beyond cin hold GARBAGE, as do the channels of rel
        w1 = D.w1.clone()
        w1[:, cin:] = GARBAGE
        rel = rel.clone()
        rel[:, cin:] = GARBAGE
    h1_ref, y2_ref, ysum, ysq = S.pos_forward(rel, w1, cin, D.s1, D.t1, D.w2, dtype)
    _fits_fp32(h1_ref, what), _fits_fp32(y2_ref, what)
    # the MFMA sums are exact: every product is a multiple of the smallest stored h1 step and the absolute row sums stay below 2^24 steps
    h1s = S.stored(h1_ref, dtype)
    step = 2.0 ** -14 if kind == "fine" else 0.5
    assert bool(((h1s / step).frac() == 0).all()) and float((h1s @ D.w2.double().abs().t()).max()) / step < U24
    rows = L.load().rv_pos_forward_rows(p)
    ktm = 128 * 256 // c
    steps = (p + ktm - 1) // ktm
    assert rows == min(256, (p + 127) // 128)
    if with_stats:
        per_row = ((steps + rows - 1) // rows) * ktm
        _row_sums_exact(float(y2_ref.abs().max()) ** 2, min(p, per_row), step * step, what)
    h1, y2 = _Out(p, c, dtype), _Out(p, c, dtype)
    partial = _nan(rows + L.STATS_SCRATCH_ROWS, 2, c) if with_stats else None
    _call(dtype, "rv_pos_forward", L.ptr(rel), ld_rel, cin, p, L.ptr(w1), 8, L.ptr(D.s1), L.ptr(D.t1), L.ptr(D.w2), c,
          L.ptr(h1.view), L.ptr(y2.view), L.ptr(partial), L.stream_ptr())
    _sync()
    h1.check(h1_ref, what + " h1")
    y2.check(y2_ref, what + " y2")
    if with_stats:
        if steps < rows:
            assert bool((partial[steps:rows] == 0).all()), what + ": the row of an idle workgroup is not zero"
        _check_partial(partial, rows, ysum, ysq, what + " statistics")
    return h1, y2, h1_ref, y2_ref


def _pos_p_list(c):
    ktm = 128 * 256 // c
    return [1, ktm - 1, ktm, ktm + 1, 999, 256 * ktm + 1]


POS_FWD_CASES = [(c, p, dtype) for c in (256, 128) for p in _pos_p_list(c) for dtype in (BF16, F16)]


@pytest.mark.parametrize("c,p,dtype", POS_FWD_CASES, ids=[f"c{c}-p{p}-{'fp16' if d == F16 else 'bf16'}" for c, p, d in POS_FWD_CASES])
def test_pos_forward(c, p, dtype):
    """rv_pos_forward: h1 and y2 bit for bit, nothing behind row P, every partial row written (zero rows of idle workgroups included),
    the statistics those of the unrounded y2; stats_partial = NULL stores the same tensors."""
    D = _pos(c, dtype)
    i = _pos_p_list(c).index(p)
    big = p > 1000
    cin = 3 if big else (1, 2, 3)[i % 3]
    ld_rel = (4, 8, 32)[(i + (c == 128)) % 3]
    what = f"pos_forward c={c} p={p} cin={cin} ld_rel={ld_rel} {dtype}"
    h1, y2, h1_ref, _ = _run_pos_forward(D, p, cin, ld_rel, True, what)
    h1n, y2n, _, _ = _run_pos_forward(D, p, cin, ld_rel, False, what + " no statistics")
    assert torch.equal(h1.view, h1n.view) and torch.equal(y2.view, y2n.view)
    if p >= 999 and cin == 3:
        y1 = S.smallk_y(D.rel32[:p], D.w1, 3)
        on_zero = float(((y1 * D.s1.double() + D.t1.double()) == 0).double().mean())
        assert 0.02 < on_zero < 0.2, on_zero  # first-layer gates exactly on 0 (the h1 there is +0)


@pytest.mark.parametrize("c", [256, 128])
@pytest.mark.parametrize("kind", ["wide", "fine"])
def test_pos_forward_rounding(c, kind):
    """Rounding pinned: "wide" -- y2 beyond 256 in halves (odd values are ties), with the statistics of the unrounded values; "fine" -- h1 and
    y2 beyond 8 significant bits (no statistics: their squares would not be exact)."""
    p = 5 if kind == "wide" else 300
    D = _Pos(p, c, 3, seed=c + len(kind), kind=kind)
    _, _, h1_ref, y2_ref = _run_pos_forward(D, p, 3, 8, kind == "wide", f"pos_forward {kind} c={c}", kind=kind)
    if kind == "wide":
        assert _rounds(y2_ref, BF16) == (True, True)
    else:
        assert _rounds(h1_ref, BF16) == (True, True) and _rounds(y2_ref, BF16)[0]


POS_IMAGES = [(1, 1, 32), (3, 1, 33), (2, 5, 37), (2, 3, 300)]
POS_MOD_CASES = [(c, d, BF16) for c in (256, 128) for d in POS_IMAGES] + [(256, (3, 1, 33), F16), (128, (2, 5, 37), F16)]


@pytest.mark.parametrize("c,dims,dtype", POS_MOD_CASES, ids=[f"c{c}-{'x'.join(map(str, d))}-{'fp16' if t == F16 else 'bf16'}" for c, d, t in POS_MOD_CASES])
def test_pos_modulate_forward(c, dims, dtype):
    """The inference form against stem_ref.pos_modulate (a reference, not the kernels it replaces): geo bit for bit, pitched feat, strict
    second-layer gates, every tap outside the image exactly 0."""
    L = _L()
    n, h, w = dims
    px = n * h * w
    i = POS_IMAGES.index(dims)
    cin, ld_rel, layout = (3, 2, 3, 1)[i], (32, 8, 4, 8)[i], LAYOUTS[(i + 1) % 3]
    D = _Pos(px * 9, c, cin, seed=c + w, dtype=dtype)
    g = _Gen(w)
    feat_t = g.ints(-7, 7, (px, c)).to(dtype)
    feat, ld_feat = _place(feat_t, layout)
    rel, _ = D.rel(ld_rel)
    what = f"pos_modulate c={c} {dims} cin={cin} ld_rel={ld_rel} {layout} {dtype}"
    ref = S.pos_modulate(rel, D.w1, cin, D.s1, D.t1, D.w2, D.s2, D.t2, feat_t, dims, dtype)
    _fits_fp32(ref, what)
    y2s = S.stored(S.pos_forward(rel, D.w1, cin, D.s1, D.t1, D.w2, dtype)[1], dtype)
    assert bool((((y2s * D.s2.double() + D.t2.double()) == 0) & (S.gather9(feat_t.double(), dims).reshape(px * 9, c) != 0)).any()), what + ": no second-layer gate on 0 (data)"
    geo = _Out(px, 9 * c, dtype)
    _call(dtype, "rv_pos_modulate_forward", L.ptr(rel), ld_rel, cin, L.ptr(D.w1), 8, L.ptr(D.s1), L.ptr(D.t1), L.ptr(D.w2), c,
          L.ptr(D.s2), L.ptr(D.t2), L.ptr(feat), ld_feat, n, h, w, L.ptr(geo.view), L.stream_ptr())
    _sync()
    geo.check(ref, what)
    inside = S.gather9(torch.ones(px, 1, dtype=torch.float64, device=DEV), dims) > 0
    assert bool((geo.view[~inside.expand(px, 9, c).reshape(px, 9 * c)] == 0).all()), what + ": a tap outside the image is not exactly 0"
    if dtype == BF16:
        assert _rounds(ref, dtype) == (True, True), what + ": no rounding case (data)"


def _pos_bwd_p_list(c):
    ktm = 128 * 256 // c
    return sorted({1, ktm - 1, ktm, ktm + 1, 129, 300, 999, 256 * ktm + 1})


POS_BWD_CASES = [(c, p) for c in (256, 128) for p in _pos_bwd_p_list(c)]


@pytest.mark.parametrize("c,p", POS_BWD_CASES, ids=[f"c{c}-p{p}" for c, p in POS_BWD_CASES])
def test_pos_backward_sums(c, p):
    """rv_pos_backward_sums: the five planes and the moments of rel exactly, plane 5 zero, from a workspace full of NaN."""
    L = _L()
    lib = L.load()
    D = _pos(c)
    i = _pos_bwd_p_list(c).index(p)
    cin = 3 if p > 1000 else (3, 1, 2)[i % 3]
    ld_rel = (8, 32)[i % 2]
    what = f"pos_backward_sums c={c} p={p} cin={cin} ld_rel={ld_rel}"
    rel, _ = D.rel(ld_rel)
    rel, dy2, w1 = rel[:p], D.dy2[:p], D.w1
    if cin != 3:
        w1, rel = D.w1.clone(), rel.clone()
        w1[:, cin:] = GARBAGE
        rel[:, cin:] = GARBAGE
    g, y1 = S.pos_masked_grad(dy2, D.w2s, rel, w1, cin, D.s1, D.t1)
    s0, s1, r = S.pos_backward_planes(dy2, D.w2s, rel, w1, cin, D.s1, D.t1, D.mean1, D.invstd1)
    rows = min(rows_of(p), 256, (p + 127) // 128)  # the workgroups (= partial rows) the launcher takes
    ktm = 128 * 256 // c
    per_row = (((p + ktm - 1) // ktm + rows - 1) // rows) * ktm
    _row_sums_exact((g * R.xhat(y1, D.mean1, D.invstd1)).abs().max(), min(p, per_row), 0.25, what)
    _row_sums_exact(float(g.abs().max()) * float(rel[:, :3].abs().max()), min(p, per_row), 1.0, what)
    _row_sums_exact(float(rel[:, :4].abs().max()) ** 2, 257, 1.0, what)
    assert float((dy2.double().abs() @ D.w2s.double().abs().t()).max()) < U24
    ws = _ff_bytes(lib.rv_bn_bwd_smallk_workspace_bytes(p, c, cin))
    sums, moms = _nan(6 * c, dtype=torch.float64), _nan(20, dtype=torch.float64)
    L.call("rv_pos_backward_sums", p, c, L.ptr(dy2), L.ptr(D.w2s), L.ptr(rel), ld_rel, cin, L.ptr(w1), 8, *_ptrs(D.s1, D.t1, D.mean1, D.invstd1),
           L.ptr(sums), L.ptr(moms), L.ptr(ws), L.stream_ptr())
    _sync()
    want = torch.cat([s0, s1, r.reshape(-1)])
    got = sums[: 5 * c]
    assert torch.equal(got, want), f"{what}: planes {sorted(set(((got != want).nonzero().flatten() // c).tolist()))} differ, first channels {((got != want).nonzero().flatten() % c).tolist()[:8]}"
    assert bool((sums[5 * c:] == 0).all()), what + ": plane 5 is not zero"
    m1, m2 = S.smallk_moments(rel, 4)
    assert torch.equal(moms, torch.cat([m1, m2.reshape(-1)])), what + ": moms differ"


# ================================================================================================================== argument checks
def test_argument_checks():
    """The rejections the entry points make, as RvError and before any launch: the sentinel-filled outputs stay untouched."""
    L = _L()
    RvError = L.RvError
    G = _Gather((1, 2, 3), 8, seed=1)
    n, h, w = G.dims
    geo, dfeat, dy = _Out(G.px, 72, BF16), _Out(G.px, 8, BF16), _Out(G.px * 9, 8, BF16)
    partial = torch.full((1 + L.STATS_SCRATCH_ROWS, 2, 8), SENTINEL, device=DEV)
    p_, st = L.ptr, L.stream_ptr()

    def modulate(c, ld_feat=8, pos=G.pos):
        L.call("rv_meta_modulate", p_(pos), p_(G.scale), p_(G.shift), p_(G.feat), ld_feat, n, h, w, c, p_(geo.view), st)

    def bwd_sums(c, partial_=partial):
        L.call("rv_meta_modulate_bwd_sums", *_ptrs(G.dgeo, G.pos, G.scale, G.shift, G.mean, G.invstd, G.feat), 8, n, h, w, c, p_(dfeat.view),
               8, p_(partial_), st)

    def bwd_apply(c, coef=G.coef):
        L.call("rv_meta_modulate_bwd_apply", *_ptrs(G.dgeo, G.pos, G.scale, G.shift, G.mean, G.invstd, coef, G.feat), 8, n, h, w, c, p_(dy.view), st)

    D = _SmallK(4, 8, 3, seed=2)
    hh = _Out(4, 8, BF16)
    sums, moms = torch.full((48,), SENTINEL, dtype=torch.float64, device=DEV), torch.full((20,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = _ff_bytes(L.load().rv_bn_bwd_smallk_workspace_bytes(4, 8, 3))

    def forward(cin, c=8, v=D.v8):
        L.call("rv_smallk_forward", p_(v), 8, 4, cin, p_(D.w), 8, c, None, 0, None, None, EPS, MOM, None, None,
               p_(D.scale), p_(D.shift), None, None, 1, p_(hh.view), 8, st)

    def smallk_sums(cin, flags, w):
        L.call("rv_bn_bwd_smallk_sums", 4, 8, p_(D.dout), 8, None, 0, p_(D.y), 8, *_ptrs(D.scale, D.shift, D.mean, D.invstd), flags,
               p_(D.v8), 8, cin, p_(w), 8, p_(sums), p_(moms), p_(ws), st)

    def moments(cin, mom=moms):
        L.call("rv_smallk_moments", p_(D.v8), 8, 4, cin, p_(mom), p_(ws), st)

    P = _Pos(288, 256, 3, seed=3)
    h1, y2 = _Out(288, 256, BF16), _Out(288, 256, BF16)
    feat = torch.zeros(32, 256, dtype=BF16, device=DEV)
    sums_p = torch.full((6 * 256,), SENTINEL, dtype=torch.float64, device=DEV)
    ws_p = _ff_bytes(L.load().rv_bn_bwd_smallk_workspace_bytes(288, 256, 3))

    def pos_forward(c, cin, rel=P.rel32):
        L.call("rv_pos_forward", p_(rel), 32, cin, 288, p_(P.w1), 8, p_(P.s1), p_(P.t1), p_(P.w2), c, p_(h1.view), p_(y2.view), None, st)

    def pos_modulate(c, cin, width, feat_=feat):
        L.call("rv_pos_modulate_forward", p_(P.rel32), 32, cin, p_(P.w1), 8, p_(P.s1), p_(P.t1), p_(P.w2), c, p_(P.s2), p_(P.t2), p_(feat_), 256,
               1, 1, width, p_(y2.view), st)

    def pos_backward(c, cin, dy2=P.dy2):
        L.call("rv_pos_backward_sums", 288, c, p_(dy2), p_(P.w2s), p_(P.rel32), 32, cin, p_(P.w1), 8, *_ptrs(P.s1, P.t1, P.mean1, P.invstd1),
               p_(sums_p), p_(moms), p_(ws_p), st)

    rejected = [
        ("C % 8", lambda: modulate(12)), ("C % 8", lambda: bwd_sums(12)), ("C % 8", lambda: bwd_apply(12)), ("C % 8", lambda: forward(3, c=12)),
        ("C > 2048", lambda: modulate(2056)), ("C > 2048", lambda: bwd_sums(2056)), ("C > 2048", lambda: bwd_apply(2056)), ("C > 2048", lambda: forward(3, c=2056)),
        ("ld_feat % 8", lambda: modulate(8, ld_feat=12)),
        ("null", lambda: modulate(8, pos=None)), ("null", lambda: bwd_sums(8, partial_=None)), ("null", lambda: bwd_apply(8, coef=None)),
        ("null", lambda: forward(3, v=None)), ("null", lambda: moments(3, mom=None)), ("null", lambda: pos_forward(256, 3, rel=None)),
        ("null", lambda: pos_modulate(256, 3, 32, feat_=None)), ("null", lambda: pos_backward(256, 3, dy2=None)),
        ("c not 128 / 256", lambda: pos_forward(64, 3)), ("c not 128 / 256", lambda: pos_forward(512, 3)), ("c not 128 / 256", lambda: pos_modulate(192, 3, 32)),
        ("c not 128 / 256", lambda: pos_backward(64, 3)),
        ("cin", lambda: pos_forward(256, 0)), ("cin", lambda: pos_forward(256, 4)), ("cin", lambda: pos_modulate(256, 4, 32)), ("cin", lambda: pos_backward(256, 4)),
        ("cin", lambda: forward(0)), ("cin", lambda: forward(9)), ("cin", lambda: moments(0)), ("cin", lambda: moments(9)),
        ("cin", lambda: smallk_sums(9, S.BNB_Y_FROM_INPUT, D.w)), ("cin", lambda: smallk_sums(0, 0, D.w)),
        ("W < 32", lambda: pos_modulate(256, 3, 31)),
        ("Y_FROM_INPUT without the weight", lambda: smallk_sums(3, S.BNB_Y_FROM_INPUT, None)),
    ]
    for why, launch in rejected:
        with pytest.raises(RvError):
            launch()
            pytest.fail(f"not rejected: {why}")
    _sync()
    for o in (geo, dfeat, dy, hh, h1, y2):
        o.untouched("argument checks")
    assert bool((partial == SENTINEL).all()) and bool((sums == SENTINEL).all()) and bool((moms == SENTINEL).all()) and bool((sums_p == SENTINEL).all())
    assert bool((ws == 255).all()) and bool((ws_p == 255).all())
