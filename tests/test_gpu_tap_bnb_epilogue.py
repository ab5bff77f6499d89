"""``rv_tap_data_grad_bnb`` at the C ABI: the ``EPI == 1`` epilogue of tapconv5.hip / tapconv6.hip -- a backward-data launch that also forms
the BatchNorm-backward sums (sum g, sum g*xhat) of the layer whose output gradient it writes -- in every form of its partial rows, exactly.

Method (test_gpu_tapconv4/5/6.py, test_gpu_wgrad3.py): integer ``dout`` (-3..3), weights (-1..1) and ``y`` (-2..2), ``scale`` in {1/2, 1, 2},
integer ``shift`` and ``mean``, ``invstd`` in {1/2, 1}.  ``dx`` is an integer below 2^24 rounded once to bf16 (two cases with 256 source
channels reach |dx| > 256, where that rounding acts, and the sums must be those of the STORED values); every term of the two sums is
an integer or a half-integer, and ``fused_bnb_ref.exactness_margin`` (asserted on the reference alone, first) keeps the sum of their
absolute values below 2^23: every fp32 partial sum is exact in any order, so the comparison is ``torch.equal``.  An integer shift puts
about 15 % of the elements on ``t == scale*y+shift == 0`` exactly (asserted > 1 %): the gate is a strict ``>``.  ``dx``, the pad columns of
``y`` and ``partial`` are pre-filled with NaN: a row that is never written, a read of a pad column or a write past ``rows`` shows.

Every case asserts: ``rv_tap_launch_info`` = the intended generation; ``rv_tap_bnb_rows`` = the row count of the intended form (below) and
the rows the test reads; ``dx`` == the CPU convolution rounded once to bf16 == a plain ``rv_tap_scatter`` / ``rv_tap_gather`` launch of the
same arguments, bit for bit; all ``rows x 2 x C_dst`` values finite and their fp64 row sums == ``data_grad_bnb_ref`` of the stored ``dx``;
the ``RV_STATS_SCRATCH_ROWS`` behind them still NaN.

Forms (``info`` = rv_tap_launch_info's {generation, channels per workgroup, pixel tiles, channel tiles}; cu = ``E.cu_count``):

* ``wg``   generation 6, one row per workgroup slot: ``rows == grid / info[3]`` with ``grid = 8 * ceil(info[2] / 8) * info[3]`` (<= cu) or the
  persistent ``cu & ~7``.  Small grids (2 x 17 x 40 and 3 x 17 x 40, ragged rows and columns, 1 / 2 / 3 channel tiles): every workgroup has
  at most one tile and ``rows == 8 * ceil(info[2] / 8)``; at 3 x 17 x 40 that is 16 rows for 12 tiles -- four workgroups per channel tile
  own no tile and must write ZERO rows (asserted ``rows > info[2]``).  Persistent (``info[2] * info[3]`` 10-30 % above cu: 3 x 48 x 1024
  x 128 channels = 288 tiles, 3 x 48 x 512 x 256 channels = 144 x 2): ``rows < info[2]``, a workgroup adds several tiles up in LDS.
* ``tile`` generation 6, one row per tile under a persistent grid: 128 k channels with k the first of (3, 5, 7) that does not divide
  ``(cu & ~7) / 8`` (3 on an MI355X), 2 x 48 x 512 = 96 tiles x 3 > cu: ``rows == info[2]``.  (The forward RV_OUT_STATS rows of the same
  shape: test_gpu_tapconv6.py::test_gather_3x3_exact.)
* ``tile5`` generation 5 (RV_SEL_NO_GEN6), always one row per tile, ``rows == info[2]``: 256- and 128-channel workgroups, small ragged
  (12 tiles on 16 workgroups) and persistent (3 x 24 x 1024 = 288 tiles of 8 x 32 pixels, one walk of ``cu & ~7`` workgroups).

Geometries.  Backward-data of a 3x3 Conv2d is the SCATTER form (cases above); the input gradient of a stride-1 ConvTranspose2d((3, 3),
padding 1) is the GATHER form (both generations).  tests/golden/tap_plan_census.json records ``bnb_rows > 0`` for these further
(geometry, form) pairs, each run here once on the small ragged shape: scatter (3, 4) stride 2 (two phases of six taps) and (3, 8) stride 4
(four phases) on generations 6 and 5; the six-tap (3, 2) kernels -- Conv2dSame's padding (1, 0) and the folded view's (1, 1) -- in both
forms on generation 6; the three-tap (3, 1) and (1, 3) kernels, which only generation 5's 256-channel tile takes (gather; (3, 1) also
scatter).  The census holds no other geometry with fused sums.

Refusals: RV_OUT_ACCUM in the shape flags (``rv_tap_bnb_rows == 0``, the call fails with the documented message, nothing is written),
``ld_y < C_dst`` and ``ld_y % 8 != 0`` (rejected before any launch).
"""

from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

import fused_bnb_ref as R
from test_gpu_forward import DEV
from test_gpu_tapconv4 import _ints

pytestmark = pytest.mark.gpu

G33 = (3, 3, 1, 1, 1)  # (kh, kw, stride_w, pad_h, pad_w)
NAN = float("nan")


def _sel(gen):
    from range_view_3d_detection_amd import _lib as L

    return L.SEL_SMALL_GRIDS | (L.SEL_SMALL_GRIDS6 if gen == 6 else L.SEL_NO_GEN6)


def _persistent_shape(cu, n_tiles, tile_rows):
    """(N, H, W) whose pixel tiles (tile_rows x 32) times the channel tiles exceed the compute units by 10 to 30 %."""
    for W in (512, 1024, 256, 2048):
        for N in (2, 3, 4, 1):
            for hr in (3, 2, 4, 1):
                if 1.1 * cu <= N * hr * (W // 32) * n_tiles <= 1.3 * cu:
                    return N, hr * tile_rows, W
    raise AssertionError(f"no persistent shape for {cu} compute units")


def _operands(geom, form, c_src, c_dst, N, H, Wu, seed):
    """Integer dout / weights and the CPU result: T is the torch-layout weight [cu][cv][kh][kw] of include/rv3d.h."""
    kh, kw, s, ph, pw = geom
    g = torch.Generator().manual_seed(seed)
    scatter = form == "scatter"
    cu, cv = (c_src, c_dst) if scatter else (c_dst, c_src)
    T = _ints((cu, cv, kh, kw), g, -1, 2)
    dout = _ints((N, c_src, H, Wu if scatter else Wu * s), g)
    if scatter:  # V[h, wv] = sum T[cu][cv][ky][kx] U[h - ky + pad_h, wu], wu * s + kx - pad_w == wv
        full = F.conv_transpose2d(dout, T, stride=(1, s))
        ref = full[:, :, ph:ph + H, pw:pw + Wu * s]
    else:        # U[h, wu] = sum T[cu][cv][ky][kx] V[h + ky - pad_h, wu * s + kx - pad_w]
        ref = F.conv2d(F.pad(dout, [pw, kw - 1 - pw, ph, kh - 1 - ph]), T, stride=(1, s))
    assert ref.shape == (N, c_dst, H, Wu * s if scatter else Wu) and float(ref.abs().max()) < 2 ** 24
    return g, T, dout, ref.contiguous()


def _nan_act(N, H, W, c, ld=None):
    from range_view_3d_detection_amd import engine as E

    data = torch.full((N, H, W, ld or c), NAN, dtype=torch.bfloat16, device=DEV)
    return E.Act(data[..., :c], c) if ld else E.Act(data, c)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(geom, form, c_src, c_dst, N, H, Wu, gen, relu_z, ld_y_pad, seed):
    """One fused launch and one plain launch of the same arguments; returns everything the assertions need."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    kh, kw, s, ph, pw = geom
    scatter = form == "scatter"
    g, T, dout, ref = _operands(geom, form, c_src, c_dst, N, H, Wu, seed)
    Wd = ref.shape[3]
    y = _ints((N, H, Wd, c_dst), g, -2, 3)
    scale, shift, mean, invstd = R.data_grad_bn(c_dst, g)
    dx_stored = ref.bfloat16().double().permute(0, 2, 3, 1)
    want = R.data_grad_bnb_ref(dx_stored, y, scale, shift, mean, invstd, relu_z)
    margin = R.exactness_margin(dx_stored * R.gate(y, scale, shift, relu_z), (y.double() - mean) * invstd)
    R.assert_exact(margin)  # (on the reference alone: every fp32 partial sum is exact)
    on_zero = float(((scale * y.double() + shift) == 0).double().mean())
    assert on_zero > 0.01, on_zero

    layer = E.TapLayer(torch.nn.Parameter(T.to(DEV)), s, (ph, pw), transposed=False)
    src = E.Act.from_nchw(dout.to(DEV))
    ya = _nan_act(N, H, Wd, c_dst, c_dst + ld_y_pad)
    ya.data.copy_(y.to(DEV))
    vec = [v.float().to(DEV) for v in (scale, shift, mean, invstd)]
    with L.select(_sel(gen)):
        shape = L.TapShape(N, H, Wu, Wu * s, src.ld, c_dst, 0)
    lib = L.load()
    info = (ctypes.c_int32 * 4)()
    assert lib.rv_tap_launch_info(ctypes.byref(layer.geom), ctypes.byref(shape), int(scatter), info) == 0
    rows = lib.rv_tap_bnb_rows(ctypes.byref(layer.geom), ctypes.byref(shape), int(scatter))
    assert info[0] == gen and rows > 0, (list(info), rows)
    partial = torch.full((rows + L.STATS_SCRATCH_ROWS, 2, c_dst), NAN, dtype=torch.float32, device=DEV)
    epi = L.BnbEpilogue(ya.ptr(), ya.ld, L.BNB_RELU_Z if relu_z else 0, *[L.ptr(v) for v in vec], L.ptr(partial))
    wp = layer.packed(form)
    fused, plain = _nan_act(N, H, Wd, c_dst), _nan_act(N, H, Wd, c_dst)
    L.call("rv_tap_data_grad_bnb", ctypes.byref(layer.geom), ctypes.byref(shape), int(scatter), src.ptr(), L.ptr(wp), fused.ptr(),
           ctypes.byref(epi), L.stream_ptr())
    L.call("rv_tap_" + form, ctypes.byref(layer.geom), ctypes.byref(shape), src.ptr(), None, None, L.ptr(wp), None, plain.ptr(), None, L.stream_ptr())
    torch.cuda.synchronize()
    return dict(info=list(info), rows=rows, partial=partial.cpu(), fused=fused.data.cpu(), plain=plain.data.cpu(), ref=ref, want=want,
                cu=E.cu_count(DEV), rounded=int((ref.bfloat16().float() != ref).sum()))


def _check(r, rows_form):
    info, rows, partial, cu = r["info"], r["rows"], r["partial"], r["cu"]
    tiles, ny = info[2], info[3]
    # ---- the kernel form -------------------------------------------------------------------------------------------------------
    if rows_form in ("wg", "wg-idle", "wg-persistent"):
        grid = 8 * ((tiles + 7) // 8) * ny
        if grid > cu:
            grid = cu & ~7
        assert (grid // 8) % ny == 0 and rows == grid // ny, (info, rows)
        if rows_form == "wg-idle":
            assert grid <= cu and rows > tiles, (info, rows)       # workgroups without a tile: zero rows
        if rows_form == "wg-persistent":
            assert 1.1 * cu <= tiles * ny <= 1.3 * cu and rows < tiles, (info, rows, cu)  # several tiles per workgroup, summed in LDS
    elif rows_form == "tile":
        assert tiles * ny > cu and ((cu & ~7) // 8) % ny != 0 and rows == tiles, (info, rows, cu)
    else:
        assert rows_form == "tile5" and rows == tiles, (info, rows)
    # ---- dx: the CPU convolution rounded once, and the plain launch ---------------------------------------------------------------
    want_dx = r["ref"].bfloat16().permute(0, 2, 3, 1)
    assert torch.equal(_bits(r["fused"]), _bits(want_dx))
    assert torch.equal(_bits(r["fused"]), _bits(r["plain"]))
    # ---- every row written, the sums exact, the tail untouched ------------------------------------------------------------------
    assert bool(torch.isfinite(partial[:rows]).all()), int((~torch.isfinite(partial[:rows])).sum())
    got = partial[:rows].double().sum(0)
    assert torch.equal(got[0], r["want"][0]), float((got[0] - r["want"][0]).abs().max())
    assert torch.equal(got[1], r["want"][1]), float((got[1] - r["want"][1]).abs().max())
    assert bool(torch.isnan(partial[rows:]).all())


# (geometry, form, C_src, C_dst, (N, H, Wu), generation, relu_z, pad columns of y, rows form)
SMALL = [
    pytest.param(G33, "scatter", 64, 128, (2, 17, 40), 6, 1, 0, "wg", id="gen6-128-2x17x40"),
    pytest.param(G33, "scatter", 64, 128, (3, 17, 40), 6, 1, 8, "wg-idle", id="gen6-128-3x17x40-idle-workgroups-padded-y"),
    pytest.param(G33, "scatter", 64, 128, (2, 17, 40), 6, 0, 8, "wg", id="gen6-128-2x17x40-no-relu-padded-y"),
    pytest.param(G33, "scatter", 64, 256, (2, 17, 40), 6, 1, 8, "wg", id="gen6-256-2x17x40-padded-y"),
    pytest.param(G33, "scatter", 64, 256, (3, 17, 40), 6, 0, 0, "wg-idle", id="gen6-256-3x17x40-idle-workgroups-no-relu"),
    pytest.param(G33, "scatter", 64, 384, (2, 17, 40), 6, 1, 0, "wg", id="gen6-384-2x17x40"),
    pytest.param(G33, "scatter", 64, 384, (3, 17, 40), 6, 1, 8, "wg-idle", id="gen6-384-3x17x40-idle-workgroups-padded-y"),
    pytest.param(G33, "scatter", 64, 256, (2, 17, 40), 5, 1, 8, "tile5", id="gen5-256-2x17x40-padded-y"),
    pytest.param(G33, "scatter", 64, 256, (2, 17, 40), 5, 0, 0, "tile5", id="gen5-256-2x17x40-no-relu"),
    pytest.param(G33, "scatter", 64, 128, (2, 17, 40), 5, 1, 8, "tile5", id="gen5-128-2x17x40-padded-y"),
    # 256 source channels: |dx| passes 256, where bf16 holds every second integer -- the sums are those of the ROUNDED values
    pytest.param(G33, "scatter", 256, 128, (2, 17, 40), 6, 1, 0, "wg", id="gen6-128-2x17x40-rounded-dx"),
    pytest.param(G33, "scatter", 256, 256, (2, 17, 40), 5, 1, 0, "tile5", id="gen5-256-2x17x40-rounded-dx"),
    # the gather form: input gradient of a stride-1 ConvTranspose2d((3, 3), padding 1)
    pytest.param(G33, "gather", 64, 128, (2, 17, 40), 6, 1, 8, "wg", id="gather-gen6-128"),
    pytest.param(G33, "gather", 64, 256, (2, 17, 40), 5, 1, 0, "tile5", id="gather-gen5-256"),
    # the other (geometry, form) pairs with fused sums in tests/golden/tap_plan_census.json
    pytest.param((3, 4, 2, 1, 1), "scatter", 64, 128, (2, 17, 40), 6, 1, 8, "wg", id="scatter-3x4-stride2-gen6"),
    pytest.param((3, 8, 4, 1, 2), "scatter", 64, 128, (2, 17, 40), 6, 1, 0, "wg", id="scatter-3x8-stride4-gen6"),
    pytest.param((3, 4, 2, 1, 1), "scatter", 64, 256, (2, 17, 40), 5, 1, 0, "tile5", id="scatter-3x4-stride2-gen5-256"),
    pytest.param((3, 8, 4, 1, 2), "scatter", 64, 128, (2, 17, 40), 5, 1, 8, "tile5", id="scatter-3x8-stride4-gen5-128"),
    pytest.param((3, 2, 1, 1, 0), "gather", 64, 128, (2, 17, 40), 6, 1, 0, "wg", id="gather-3x2-same-gen6"),
    pytest.param((3, 2, 1, 1, 0), "scatter", 64, 128, (2, 17, 40), 6, 1, 8, "wg", id="scatter-3x2-same-gen6"),
    pytest.param((3, 2, 1, 1, 1), "gather", 64, 128, (2, 17, 40), 6, 0, 8, "wg", id="gather-3x2-folded-gen6"),
    pytest.param((3, 2, 1, 1, 1), "scatter", 64, 128, (2, 17, 40), 6, 1, 0, "wg", id="scatter-3x2-folded-gen6"),
    pytest.param((3, 1, 1, 1, 0), "gather", 64, 256, (2, 17, 40), 5, 1, 8, "tile5", id="gather-3x1-gen5-256"),
    pytest.param((1, 3, 1, 0, 1), "gather", 64, 256, (2, 17, 40), 5, 1, 0, "tile5", id="gather-1x3-gen5-256"),
    pytest.param((3, 1, 1, 1, 0), "scatter", 64, 256, (2, 17, 40), 5, 1, 0, "tile5", id="scatter-3x1-gen5-256"),
]


@pytest.mark.parametrize("geom,form,c_src,c_dst,nhw,gen,relu_z,ld_y_pad,rows_form", SMALL)
def test_small_grid_sums_exact(geom, form, c_src, c_dst, nhw, gen, relu_z, ld_y_pad, rows_form):
    r = _launch(geom, form, c_src, c_dst, *nhw, gen, relu_z, ld_y_pad, seed=c_dst + 7 * gen + nhw[0] + geom[1])
    assert c_src < 256 or r["rounded"] > 10, r["rounded"]  # (elements whose bf16 rounding changes the value)
    _check(r, rows_form)


@pytest.mark.parametrize("c_dst,relu_z,ld_y_pad", [(128, 1, 0), (256, 1, 8)])
def test_generation_6_persistent_workgroups_add_their_tiles_up(c_dst, relu_z, ld_y_pad):
    """``stats_per_wg == 1`` under a persistent grid: the sums of a workgroup's tiles are accumulated in LDS (``+=``) and written once."""
    from range_view_3d_detection_amd import engine as E

    N, H, W = _persistent_shape(E.cu_count(DEV), c_dst // 128, 16)
    _check(_launch(G33, "scatter", 32, c_dst, N, H, W, 6, relu_z, ld_y_pad, seed=c_dst), "wg-persistent")


def test_generation_6_per_tile_rows_under_a_persistent_grid():
    """``stats_per_wg == 0``: C_dst / 128 does not divide grid / 8, so a workgroup's tiles belong to different channel tiles and every
    tile writes its own row."""
    from range_view_3d_detection_amd import engine as E

    cu = E.cu_count(DEV)
    k = next(k for k in (3, 5, 7) if ((cu & ~7) // 8) % k != 0)
    N, H, W = _persistent_shape(cu, k, 16)
    _check(_launch(G33, "scatter", 32, 128 * k, N, H, W, 6, 1, 8, seed=k), "tile")


@pytest.mark.parametrize("c_dst", [256, 128])
def test_generation_5_persistent_loop(c_dst):
    from range_view_3d_detection_amd import engine as E

    cu = E.cu_count(DEV)
    N, H, W = _persistent_shape(cu, 1, 8)
    r = _launch(G33, "scatter", 64, c_dst, N, H, W, 5, 1, 8 if c_dst == 128 else 0, seed=c_dst + 1)
    assert r["info"][1] == c_dst and r["info"][2] * r["info"][3] > cu  # (one walk of cu & ~7 workgroups over the tiles)
    _check(r, "tile5")


def _refusal_setup(flags):
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    g = torch.Generator().manual_seed(1)
    N, H, W, c_src, c_dst = 2, 17, 40, 64, 128
    layer = E.TapLayer(torch.nn.Parameter(_ints((c_src, c_dst, 3, 3), g, -1, 2).to(DEV)), 1, (1, 1), transposed=False)
    src = E.Act.from_nchw(_ints((N, c_src, H, W), g).to(DEV))
    with L.select(_sel(6)):
        shape = L.TapShape(N, H, W, W, src.ld, c_dst, flags)
    dx = _nan_act(N, H, W, c_dst)
    ya = E.Act.from_nchw(_ints((N, c_dst, H, W), g, -2, 3).to(DEV))
    vec = [v.float().to(DEV) for v in R.data_grad_bn(c_dst, g)]
    partial = torch.full((16 + L.STATS_SCRATCH_ROWS, 2, c_dst), NAN, dtype=torch.float32, device=DEV)

    def call(ld_y):
        epi = L.BnbEpilogue(ya.ptr(), ld_y, L.BNB_RELU_Z, *[L.ptr(v) for v in vec], L.ptr(partial))
        L.call("rv_tap_data_grad_bnb", ctypes.byref(layer.geom), ctypes.byref(shape), 1, src.ptr(), L.ptr(layer.packed("scatter")), dx.ptr(),
               ctypes.byref(epi), L.stream_ptr())

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(dx.data).all()) and bool(torch.isnan(partial).all())

    return layer, shape, call, untouched, c_dst


def test_an_accumulating_launch_is_refused_and_writes_nothing():
    from range_view_3d_detection_amd import _lib as L

    layer, shape, call, untouched, c_dst = _refusal_setup(L.OUT_ACCUM)
    assert L.load().rv_tap_bnb_rows(ctypes.byref(layer.geom), ctypes.byref(shape), 1) == 0
    with pytest.raises(L.RvError, match="no fused BatchNorm-backward sums"):
        call(c_dst)
    assert untouched()


@pytest.mark.parametrize("ld_y", [120, 132])  # below C_dst; no multiple of 8
def test_a_bad_stride_of_y_is_rejected_before_any_launch(ld_y):
    from range_view_3d_detection_amd import _lib as L

    layer, shape, call, untouched, c_dst = _refusal_setup(0)
    assert L.load().rv_tap_bnb_rows(ctypes.byref(layer.geom), ctypes.byref(shape), 1) > 0
    with pytest.raises(L.RvError, match="bad channel stride of y"):
        call(ld_y)
    assert untouched()
