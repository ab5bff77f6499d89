"""The register-staged tap-conv kernels -- generation 2 (``tapconv2_kernel<KS>``: 2 rows x 64 columns x 128 channels) and generation 1
(``tapconv_kernel<M,N>``, the generic kernel) -- and the weight-gradient generations 1 and 2: exact checks with integer data at
the shapes the base-av2 / base-waymo models (BASIC stem, layers [64, 64, 128, 128, 128], towers 128) produce.

In rv-av2 / rv-waymo these kernels only see the 1/16-resolution stage and thin layers; in the base models every layer with 64
output channels runs on them at full resolution (half of tapconv2's channel tile empty, 4096-workgroup grids), reads its input
through the folded BatchNorm + ReLU prologue, and the stem writes one half of a 128-channel buffer.

Method of test_gpu_tapconv4/5/6.py: small-integer operands make every partial sum an integer below 2^24, so the output must
equal the CPU fp32 convolution rounded once to the storage type, bit for bit, whatever the summation order.  Every case asserts the
generation (``rv_tap_launch_info`` / ``rv_tap_wgrad_info``) on the very shape it launches: a selection change cannot silently move a
case to another kernel.  The launches go through the C ABI directly (``rv_tap_gather`` / ``rv_tap_scatter`` / ``rv_tap_residual`` /
``rv_tap_wgrad``), with the packed weight images of ``engine.tap_layer``.
"""

from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_forward import DEV
from test_gpu_tapconv4 import _ints

pytestmark = pytest.mark.gpu

SENTINEL = 77.0  # canary value of the channels a launch must not touch (exact in bf16 and fp16)


def _info(layer, shape, scatter):
    from range_view_3d_detection_amd import _lib as L

    info = (ctypes.c_int32 * 4)()
    assert L.load().rv_tap_launch_info(ctypes.byref(layer.geom), ctypes.byref(shape), 1 if scatter else 0, info) == 0
    return list(info)


def _tap(layer, form, src, dst=None, flags=0, scale=None, shift=None, stats=False, expect=(2, None), out_f32=False, residual=None):
    """One tap-conv launch through the C ABI.  ``src`` / ``dst`` / ``residual``: ``engine.Act`` (possibly channel slices of wider buffers).
    Returns (NCHW float result on the CPU, partial-statistics rows or None, launch info)."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    g = layer.geom
    scatter = form == "scatter"
    wu, wv = (src.W, src.W * g.stride_w) if scatter else (src.W // g.stride_w, src.W)
    c_out = layer.geom.cv if scatter else layer.geom.cu
    if out_f32:
        out_t = torch.full((src.N, src.H, wv if scatter else wu, E.pad32(c_out)), float("nan"), dtype=torch.float32, device=src.data.device)
        dst_ptr, ld_dst = L.ptr(out_t), out_t.stride(2)
        flags |= L.OUT_F32
    else:
        if dst is None:
            dst = E.Act.empty(src.N, src.H, wv if scatter else wu, c_out, src.data.device)
        dst_ptr, ld_dst = dst.ptr(), dst.ld
    bias = None
    if layer.bias is not None:
        flags |= L.OUT_BIAS
        bias = layer.padded_bias()
    shape = L.TapShape(src.N, src.H, wu, wv, src.ld, ld_dst, flags | (L.OUT_STATS if stats else 0))
    info = _info(layer, shape, scatter)
    assert info[0] == expect[0] and (expect[1] is None or info[1] == expect[1]), (info, expect)
    partial = None
    if stats:
        rows = L.load().rv_tap_stats_rows(ctypes.byref(g), ctypes.byref(shape), 1 if scatter else 0)
        assert rows > 0
        # NaN-filled: a (row, channel) the launch leaves unwritten shows in the sums
        partial = torch.full((rows + L.STATS_SCRATCH_ROWS, 2, E.pad32(c_out)), float("nan"), dtype=torch.float32, device=src.data.device)
    wp = layer.packed(form)
    if residual is not None:
        L.call("rv_tap_residual", ctypes.byref(g), ctypes.byref(shape), 1 if scatter else 0, src.ptr(), L.ptr(wp), L.ptr(bias),
               residual.ptr(), residual.ld, dst_ptr, L.stream_ptr())
    else:
        L.call("rv_tap_" + form, ctypes.byref(g), ctypes.byref(shape), src.ptr(), L.ptr(scale), L.ptr(shift), L.ptr(wp), L.ptr(bias),
               dst_ptr, L.ptr(partial), L.stream_ptr())
    torch.cuda.synchronize()
    got = (out_t if out_f32 else dst.data)[..., :c_out].permute(0, 3, 1, 2).float().cpu()
    return got, (partial[:rows] if stats else None), info


def _conv(cin, cout, k, g, bias=False, stride=1):
    from range_view_3d_detection_amd import engine as E

    m = torch.nn.Conv2d(cin, cout, k, stride=(1, stride), padding=k // 2, bias=bias)
    m.weight.data = _ints(m.weight.shape, g, -2, 3)
    if bias:
        m.bias.data = _ints(m.bias.shape, g, -8, 9)
    m = m.to(DEV)
    return m, E.tap_layer(m)


def _act(x):
    from range_view_3d_detection_amd import engine as E

    return E.Act.from_nchw(x.to(DEV))


def _check_stats(partial, ref, cout):
    rows = partial.double().sum(dim=0).cpu()  # (2, C_pad): NaN anywhere = an unwritten (row, channel)
    assert torch.isfinite(rows).all()
    assert torch.allclose(rows[0, :cout], ref.double().sum(dim=(0, 2, 3)), rtol=1e-6, atol=1e-3)
    assert torch.allclose(rows[1, :cout], (ref.double() ** 2).sum(dim=(0, 2, 3)), rtol=1e-5)
    assert not rows[:, cout:].any()  # padding channels (zero weights) sum to zero


# ------------------------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("cin,cout,N,H,W,ks", [(64, 64, 4, 64, 2048, 2),   # res1 of base-av2 at full size: 4096 workgroups, half of the channel tile empty
                                               (64, 64, 2, 64, 2656, 2),   # base-waymo: 41 whole column tiles + one of 32
                                               (64, 64, 3, 17, 333, 2),    # odd H (one-row last tile row), ragged columns
                                               (64, 64, 5, 2, 64, 2),      # one tile per image
                                               (64, 96, 2, 9, 200, 2),     # 96 of 128 channels
                                               (64, 160, 2, 9, 200, 2),    # a whole channel tile and a ragged second one
                                               (32, 64, 2, 9, 200, 1),     # one 32-channel chunk: the <1> variant
                                               (192, 64, 2, 9, 200, 2)])   # three chunks
def test_gather_3x3_exact(cin, cout, N, H, W, ks):
    g = torch.Generator().manual_seed(cin + cout + W)
    m, layer = _conv(cin, cout, 3, g)
    x = _ints((N, cin, H, W), g)
    ref = F.conv2d(x, m.weight.data.cpu(), padding=1)
    got, partial, info = _tap(layer, "gather", _act(x), stats=True, expect=(2, ks))
    if (N, H, W) == (4, 64, 2048):
        assert info[2] == 4096 and info[3] == 1, info
    assert torch.equal(got, ref.bfloat16().float())
    _check_stats(partial, ref, cout)


@pytest.mark.parametrize("cin,cout,N,H,W,ks", [(64, 64, 4, 64, 2048, 2),   # the stem's second conv at full size (the one-tap, double-buffered form)
                                               (5, 64, 2, 64, 2656, 1),    # 5 -> 64 (input padded to 32): the stem's projection conv (no ReLU behind it: not a small-K layer)
                                               (6, 64, 3, 17, 333, 1),
                                               (64, 64, 3, 17, 333, 2)])
def test_gather_1x1_exact(cin, cout, N, H, W, ks):
    g = torch.Generator().manual_seed(cin + W)
    m, layer = _conv(cin, cout, 1, g)
    x = _ints((N, cin, H, W), g)
    ref = F.conv2d(x, m.weight.data.cpu())
    got, partial, _ = _tap(layer, "gather", _act(x), stats=True, expect=(2, ks))
    assert torch.equal(got, ref.bfloat16().float())
    _check_stats(partial, ref, cout)


@pytest.mark.parametrize("cout,N,H,W", [(26, 4, 64, 2048), (8, 2, 64, 2656), (3, 3, 17, 333)])
def test_tower_final_conv_f32_bias_exact(cout, N, H, W):
    """128 -> classes / 8 regressands, 1x1, fp32 output with bias: the generic kernel (fewer than 64 output channels)."""
    g = torch.Generator().manual_seed(cout + W)
    m, layer = _conv(128, cout, 1, g, bias=True)
    x = _ints((N, 128, H, W), g)
    ref = F.conv2d(x, m.weight.data.cpu(), m.bias.data.cpu())
    got, _, _ = _tap(layer, "gather", _act(x), expect=(1, None), out_f32=True)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------- channel slices with canaries
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("half", [0, 1])
def test_gather_into_half_of_a_128_channel_buffer_leaves_the_other_half_alone(k, half):
    """The BASIC stem writes channels [0, 64) of the level-1 feature buffer and agg3 writes [64, 128); res1 reads [0, 64) with
    ld_src = 128.  64 channels are HALF of tapconv2's channel tile: a store masked by the tile instead of by C_dst would overwrite the neighbour."""
    from range_view_3d_detection_amd import engine as E

    g = torch.Generator().manual_seed(10 * k + half)
    N, H, W = 2, 9, 200
    m, layer = _conv(64, 64, k, g)
    x = _ints((N, 64, H, W), g)
    other = _ints((N, 64, H, W), g, -9, 10)  # the half of the SOURCE buffer the launch must not read
    src_buf = _act(torch.cat([x, other] if half == 0 else [other, x], dim=1))
    dst_buf = E.Act(torch.full((N, H, W, 128), SENTINEL, dtype=torch.bfloat16, device=DEV), 128)
    ref = F.conv2d(x, m.weight.data.cpu(), padding=k // 2)
    got, _, _ = _tap(layer, "gather", src_buf.slice(64 * half, 64 * half + 64), dst=dst_buf.slice(64 * half, 64 * half + 64), expect=(2, 2))
    assert torch.equal(got, ref.bfloat16().float())
    keep = dst_buf.data[..., 64 * (1 - half) : 64 * (1 - half) + 64]
    assert torch.equal(keep, torch.full_like(keep, SENTINEL))


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("half", [0, 1])
def test_residual_epilogue_into_a_slice_leaves_the_other_half_alone(tag, half):
    """Inference: the stem's last conv adds the projection branch in its own epilogue (``rv_tap_residual``) and writes the slice;
    both operand types (the fp16 library is what evaluation under autocast(float16) runs)."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    g = torch.Generator().manual_seed(3 + half)
    N, H, W = 2, 9, 200
    with L.operand(tag):
        m, layer = _conv(64, 64, 1, g, bias=True)
        x = _ints((N, 64, H, W), g)
        res = _ints((N, 64, H, W), g, -20, 21)
        dst_buf = E.Act(torch.full((N, H, W, 128), SENTINEL, dtype=L.act_dtype(), device=DEV), 128)
        res_buf = _act(torch.cat([res, res + 1], dim=1))  # the residual is read as a slice too (ld_res = 128)
        shape_flags = L.OUT_RELU | L.OUT_RES_RELU
        got, _, _ = _tap(layer, "gather", _act(x), dst=dst_buf.slice(64 * half, 64 * half + 64), flags=shape_flags, expect=(2, 2),
                         residual=res_buf.slice(0, 64))
        store = lambda t: t.to(L.act_dtype()).float()
        ref = F.relu(store(F.relu(F.conv2d(x, m.weight.data.cpu(), m.bias.data.cpu()))) + res)
        assert torch.equal(got, store(ref))
        keep = dst_buf.data[..., 64 * (1 - half) : 64 * (1 - half) + 64]
        assert torch.equal(keep, torch.full_like(keep, SENTINEL))


@pytest.mark.parametrize("half", [0, 1])
def test_combine_into_a_slice_leaves_the_other_half_alone(half):
    """Training: the block output relu(bn(a) + bn(b)) is one element-wise pass (``rv_ew_combine``) into the slice."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    g = torch.Generator().manual_seed(half)
    N, H, W, C = 1, 27, 37, 64  # 999 pixels
    a, b = _ints((N, C, H, W), g, -6, 7), _ints((N, C, H, W), g, -6, 7)
    sa, ta = _ints((C,), g, 1, 3).to(DEV), _ints((C,), g, -4, 5).to(DEV)
    sb, tb = _ints((C,), g, 1, 3).to(DEV), _ints((C,), g, -4, 5).to(DEV)
    A, B = _act(a), _act(b)
    dst_buf = E.Act(torch.full((N, H, W, 128), SENTINEL, dtype=torch.bfloat16, device=DEV), 128)
    out = dst_buf.slice(64 * half, 64 * half + 64)
    L.call("rv_ew_combine", A.pixels, C, A.ptr(), A.ld, L.ptr(sa), L.ptr(ta), B.ptr(), B.ld, L.ptr(sb), L.ptr(tb),
           out.ptr(), out.ld, L.EW_RELU_A | L.EW_RELU_OUT, L.stream_ptr())
    torch.cuda.synchronize()
    v = lambda t: t.cpu().view(1, C, 1, 1)
    ref = F.relu(F.relu(a * v(sa) + v(ta)) + (b * v(sb) + v(tb)))
    assert torch.equal(out.nchw().float().cpu(), ref.bfloat16().float())
    keep = dst_buf.data[..., 64 * (1 - half) : 64 * (1 - half) + 64]
    assert torch.equal(keep, torch.full_like(keep, SENTINEL))


# ------------------------------------------------------------------------------------- folded BatchNorm + ReLU in the operand staging
@pytest.mark.parametrize("cin,cout,N,H,W,relu", [(64, 64, 4, 64, 2048, True), (64, 64, 3, 17, 333, True), (64, 128, 2, 9, 200, False),
                                                 (32, 64, 2, 9, 200, True)])
def test_affine_relu_prologue_exact_and_padding_stays_zero(cin, cout, N, H, W, relu):
    """operand = relu(scale[c] * x + shift[c]) formed while the tile is staged; the zero padding of the 3x3 applies to the
    TRANSFORMED tensor (shifts of both signs: a border position that went through the transform would contribute relu(shift) != 0)."""
    from range_view_3d_detection_amd import _lib as L

    g = torch.Generator().manual_seed(cin + cout + W)
    m, layer = _conv(cin, cout, 3, g)
    x = _ints((N, cin, H, W), g, -3, 4)
    scale, shift = _ints((cin,), g, 1, 3), _ints((cin,), g, -3, 4)
    assert (shift > 0).any() and (shift < 0).any()
    h = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    ref = F.conv2d(F.relu(h) if relu else h, m.weight.data.cpu(), padding=1)
    got, partial, _ = _tap(layer, "gather", _act(x), flags=L.IN_AFFINE | (L.IN_RELU if relu else 0), scale=scale.to(DEV), shift=shift.to(DEV),
                           stats=True, expect=(2, 2 if cin % 64 == 0 else 1))
    assert torch.equal(got, ref.bfloat16().float())
    _check_stats(partial, ref, cout)


# ---------------------------------------------------------------------------------------------------------------- scatter forms
@pytest.mark.parametrize("cin,cout,kernel,stride,padding,N,H,W", [(128, 64, (3, 8), 4, (1, 2), 4, 64, 512),   # agg1 of the base models at full size
                                                                   (128, 64, (3, 4), 2, (1, 1), 2, 64, 664),   # agg2a, base-waymo's W / 4
                                                                   (64, 64, (3, 4), 2, (1, 1), 4, 64, 1024),   # agg3 at full size
                                                                   (64, 64, (3, 4), 2, (1, 1), 3, 17, 83),     # ragged
                                                                   (128, 64, (3, 8), 4, (1, 2), 3, 17, 83)])
def test_conv_transpose_exact(cin, cout, kernel, stride, padding, N, H, W):
    """ConvTranspose2d forward = the scatter form, one launch over all ``stride`` output phases (2 x 3 / 2 x 6 taps per phase)."""
    from range_view_3d_detection_amd import engine as E

    g = torch.Generator().manual_seed(W + cin)
    m = torch.nn.ConvTranspose2d(cin, cout, kernel, stride=(1, stride), padding=padding, bias=False)
    m.weight.data = _ints(m.weight.shape, g, -2, 3)
    m = m.to(DEV)
    x = _ints((N, cin, H, W), g)
    ref = F.conv_transpose2d(x, m.weight.data.cpu(), stride=(1, stride), padding=padding)
    got, partial, _ = _tap(E.tap_layer(m), "scatter", _act(x), stats=True, expect=(2, 2))
    assert torch.equal(got, ref.bfloat16().float())
    _check_stats(partial, ref, cout)


@pytest.mark.parametrize("cin,cout,k,N,H,W", [(64, 64, 3, 4, 64, 1024), (64, 128, 3, 2, 64, 512), (64, 64, 1, 2, 64, 664), (64, 128, 1, 3, 17, 83)])
def test_stride2_backward_data_and_accumulate_exact(cin, cout, k, N, H, W):
    """Backward-data of the stride-2 convs (res2a.0 64 -> 64, res2.0 64 -> 128 and their 1x1 projections): the scatter form with two
    phases, into a fresh buffer and accumulating into an existing gradient (RV_OUT_ACCUM: bf16(bf16(result) + old)).  W = coarse width."""
    from range_view_3d_detection_amd import _lib as L

    g = torch.Generator().manual_seed(cout + k + W)
    m, layer = _conv(cin, cout, k, g, stride=2)
    dy = _ints((N, cout, H, W), g)
    old = _ints((N, cin, H, 2 * W), g, -20, 21)
    ref = F.conv_transpose2d(dy, m.weight.data.cpu(), stride=(1, 2), padding=k // 2, output_padding=(0, 1))
    got, _, _ = _tap(layer, "scatter", _act(dy), expect=(2, 2))
    assert torch.equal(got, ref.bfloat16().float())
    dst = _act(old)
    got, _, _ = _tap(layer, "scatter", _act(dy), dst=dst, flags=L.OUT_ACCUM, expect=(2, 2))
    assert torch.equal(got, (ref.bfloat16().float() + old).bfloat16().float())


# ------------------------------------------------------------------------------------------------------------ the generic kernel
@pytest.mark.parametrize("cin,cout,k,N,H,W", [(64, 64, 3, 4, 64, 1024),   # res2a.0 unfolded at full size: 4096 workgroups of tapconv_kernel<2,2>
                                              (64, 128, 3, 2, 64, 664),
                                              (64, 64, 1, 3, 17, 83),
                                              (64, 128, 3, 3, 17, 83)])
def test_strided_gather_on_the_generic_kernel_exact(cin, cout, k, N, H, W):
    """Stride-2 convs in their own (unfolded) geometry: what runs when the engine does not fold (``engine.FOLD_STRIDED = False``, an
    odd fine width, an affine prologue).  W = coarse width."""
    g = torch.Generator().manual_seed(cin + cout + W)
    m, layer = _conv(cin, cout, k, g, stride=2)
    x = _ints((N, cin, H, 2 * W), g)
    ref = F.conv2d(x, m.weight.data.cpu(), stride=(1, 2), padding=k // 2)
    got, partial, info = _tap(layer, "gather", _act(x), stats=True, expect=(1, None))
    if (N, H, W) == (4, 64, 1024):
        assert info[2] >= 4096, info
    assert torch.equal(got, ref.bfloat16().float())
    _check_stats(partial, ref, cout)


def test_engine_reaches_the_generic_kernel_without_folding(monkeypatch):
    """The same layer through ``engine.ConvOp`` with folding off: the launch record names the generic kernel and the result is exact."""
    from range_view_3d_detection_amd import engine as E

    monkeypatch.setattr(E, "FOLD_STRIDED", False)
    g = torch.Generator().manual_seed(2)
    m, layer = _conv(64, 64, 3, g, stride=2)
    x = _ints((2, 64, 16, 512), g)
    E.PROFILE = E.KernelProfile()
    try:
        op = E.ConvOp(E.Tape(True, DEV), layer, _act(x), stats=True)
        torch.cuda.synchronize()
        ran = [name for name, *_ in E.PROFILE.records]
    finally:
        E.PROFILE = None
    assert len(ran) == 1 and ran[0].startswith("tapconv_kernel<"), ran
    ref = F.conv2d(x, m.weight.data.cpu(), stride=(1, 2), padding=1)
    assert torch.equal(op.out.nchw().float().cpu(), ref.bfloat16().float())


# ------------------------------------------------------------------------------------------------------------- weight gradients
def _wgrad(geom, N, H, Wu, u, v, expect, flags=0, scale=None, shift=None, v_affine=0, torch_layout=True, ld_v=None, nan_workspace=False):
    """One ``rv_tap_wgrad`` launch through the C ABI.  ``u`` / ``v``: ``engine.Act`` (possibly channel slices of wider buffers); ``ld_v``: pixel
    stride of V when it is not ``v.ld`` (the folded view of a strided layer); ``nan_workspace``: the split-K slabs start as NaN instead of
    whatever the allocator hands out, so a slab region that no workgroup writes shows in the result."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    shape = L.TapShape(N, H, Wu, Wu * geom.stride_w, 0, 0, flags | (L.WGRAD_TORCH_LAYOUT if torch_layout else 0))
    info = (ctypes.c_int32 * 4)()
    L.call("rv_tap_wgrad_info", ctypes.byref(geom), ctypes.byref(shape), info)
    assert info[0] == expect, list(info)
    ws_bytes = L.load().rv_tap_wgrad_workspace_bytes(ctypes.byref(geom), ctypes.byref(shape))
    if nan_workspace:
        ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    else:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    cu, cv, taps = geom.cu, geom.cv, geom.kh * geom.kw
    out = torch.full((cu, cv, geom.kh, geom.kw) if torch_layout else (taps, E.pad32(cu), E.pad32(cv)), float("nan"), dtype=torch.float32, device=DEV)
    L.call("rv_tap_wgrad", ctypes.byref(geom), ctypes.byref(shape), u.ptr(), u.ld, v.ptr(), v.ld if ld_v is None else ld_v, L.ptr(scale),
           L.ptr(shift), v_affine, L.ptr(out), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    out = out.cpu()
    if not torch_layout:  # packed [tap][cu_pad][cv_pad]: padding entries are zero, the rest is the torch layout transposed
        assert not out[:, cu:].any() and not out[:, :, cv:].any()
        out = out[:, :cu, :cv].permute(1, 2, 0).reshape(cu, cv, geom.kh, geom.kw)
    return out, list(info)


@pytest.mark.parametrize("cin,cout,k,N,H,W,affine,torch_layout", [(64, 64, 3, 4, 64, 2048, True, True),    # res1 at full size, split-K over the whole image
                                                                   (64, 64, 1, 4, 64, 2048, False, False),  # the stem's second conv, packed layout
                                                                   (5, 64, 1, 2, 64, 2656, False, True),    # the stem's projection conv
                                                                   (128, 26, 1, 4, 64, 2048, True, True),   # a tower's final conv (unfused backward)
                                                                   (64, 64, 3, 3, 17, 333, True, False),    # ragged: 5 whole 64-pixel chunks + 13 per row
                                                                   (128, 8, 1, 3, 17, 333, False, True),
                                                                   (64, 96, 3, 2, 9, 200, False, True)])
def test_wgrad2_exact(cin, cout, k, N, H, W, affine, torch_layout):
    """Weight gradient of stride-1 layers that are not 128 x 128-tileable: generation 2 (register-staged three-tap groups, split-K
    + reduce), with and without the folded BatchNorm + ReLU applied to the forward input, in both result layouts.  Values in
    {-1, 0, 1} (prologue: {0, 1, 2}): every sum over the 524 288 pixels of a full-size image stays below 2^24."""
    from range_view_3d_detection_amd import _lib as L

    g = torch.Generator().manual_seed(cin + cout + W)
    m, layer = _conv(cin, cout, k, g)
    x = _ints((N, cin, H, W), g, -1, 2)
    dy = _ints((N, cout, H, W), g, -1, 2)
    scale, shift = torch.ones(cin), _ints((cin,), g, -1, 2)
    xin = F.relu(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) if affine else x
    ref = torch.nn.grad.conv2d_weight(xin, m.weight.shape, dy, padding=k // 2)
    pad = lambda t: F.pad(t, (0, (-t.numel()) % 32)).to(DEV)
    got, info = _wgrad(layer.geom, N, H, W, _act(dy), _act(x), 2, flags=(L.IN_AFFINE | L.IN_RELU) if affine else 0,
                       scale=pad(scale) if affine else None, shift=pad(shift) if affine else None, v_affine=1, torch_layout=torch_layout)
    if (N, H, W) == (4, 64, 2048) and k == 3:
        assert info[1] > 1, info  # split-K really is in play
    assert torch.equal(got, ref)


@pytest.mark.parametrize("cin,cout,k,N,H,W,affine", [(64, 64, 3, 4, 64, 1024, False),   # res2a.0 unfolded, full size
                                                     (64, 128, 3, 2, 64, 664, True),
                                                     (64, 64, 1, 3, 17, 83, False),
                                                     (64, 128, 3, 3, 17, 83, True)])
def test_wgrad1_strided_exact(cin, cout, k, N, H, W, affine):
    """The generic weight-gradient kernel: stride-2 convs in their own geometry (W = coarse width)."""
    from range_view_3d_detection_amd import _lib as L

    g = torch.Generator().manual_seed(cin + cout + W + k)
    m, layer = _conv(cin, cout, k, g, stride=2)
    x = _ints((N, cin, H, 2 * W), g, -1, 2)
    dy = _ints((N, cout, H, W), g, -1, 2)
    shift = _ints((cin,), g, -1, 2)
    xin = F.relu(x + shift.view(1, -1, 1, 1)) if affine else x
    ref = torch.nn.grad.conv2d_weight(xin, m.weight.shape, dy, stride=(1, 2), padding=k // 2)
    got, _ = _wgrad(layer.geom, N, H, W, _act(dy), _act(x), 1, flags=(L.IN_AFFINE | L.IN_RELU) if affine else 0,
                    scale=torch.ones(cin, device=DEV) if affine else None, shift=shift.to(DEV) if affine else None, v_affine=1)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("cin,cout,kernel,stride,padding,N,H,W", [(128, 64, (3, 8), 4, (1, 2), 4, 64, 512), (64, 64, (3, 4), 2, (1, 1), 4, 64, 1024),
                                                                   (128, 64, (3, 4), 2, (1, 1), 3, 17, 83)])
def test_wgrad1_conv_transpose_exact(cin, cout, kernel, stride, padding, N, H, W):
    """Weight gradient of the up-sampling ConvTranspose2d layers (U = the coarse input, V = the fine output gradient)."""
    from range_view_3d_detection_amd import engine as E

    g = torch.Generator().manual_seed(W + cin + kernel[1])
    m = torch.nn.ConvTranspose2d(cin, cout, kernel, stride=(1, stride), padding=padding, bias=False).to(DEV)
    x = _ints((N, cin, H, W), g, -1, 2)
    dy = _ints((N, cout, H, W * stride), g, -1, 2)
    w = torch.zeros(m.weight.shape, requires_grad=True)
    (F.conv_transpose2d(x, w, stride=(1, stride), padding=padding) * dy).sum().backward()
    got, _ = _wgrad(E.tap_layer(m).geom, N, H, W, _act(x), _act(dy), 1)
    assert torch.equal(got, w.grad)


# ------------------------------------------------------------------------------------------------------- the small-K stem path
@pytest.mark.parametrize("cin,shape", [(5, (1, 27, 37)), (6, (1, 27, 37)), (5, (4, 64, 2048)), (6, (4, 64, 2048))])
def test_basic_stem_small_k_layer_at_64_channels(cin, shape):
    """The first layer of the BASIC stem (conv 1x1 cin -> 64, BatchNorm, ReLU on an input that needs no gradient): ``rv_smallk_forward``
    + closed-form batch statistics and ``rv_bn_bwd_smallk*`` (the raw output recomputed from the <= 8 input channels) at C = 64, 999
    pixels and a full batch, against an fp64 evaluation of the same layer on the same bf16-valued weights, input and output gradient.
    Bounds of test_small_k_fused_paths_match_unfused_and_oracle.

    The layer is driven alone: behind the whole block the gradient reaching this BatchNorm has passed the NEXT BatchNorm's backward,
    which removes its per-channel mean -- with open gates the true dbeta is then a sum of 524 288 cancelling bf16-rounded terms, and
    a comparison of it measures the rounding of the stored gradient, not this kernel (first version of this test: cosine 0.46)."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E
    from range_view_3d_detection_amd import engine_bwd
    from range_view_3d_detection_amd.nn.blocks import BasicBlock
    from test_gpu_backward import _cos
    from test_gpu_forward import rel_err

    N, H, W = shape
    torch.manual_seed(cin)
    gen = torch.Generator().manual_seed(cin + H)
    blk = BasicBlock(cin, 64, kernel_size=1, project=True)
    conv, bn = blk.net[0].conv, blk.net[1]
    conv.weight.data = conv.weight.data.bfloat16().float()
    bn.weight.data = 0.5 + torch.rand(64, generator=gen)
    bn.bias.data = 0.3 * torch.randn(64, generator=gen) + 1.0  # (a few per cent of the gates closed: the mask matters)
    x = (torch.randn(N, cin, H, W, generator=gen) + 0.5).bfloat16().float()
    probe = (torch.randn(N, 64, H, W, generator=gen) + 0.5).bfloat16().float()
    w64 = conv.weight.data.double().requires_grad_(True)
    gamma, beta = bn.weight.data.double().requires_grad_(True), bn.bias.data.double().requires_grad_(True)
    y = F.conv2d(x.double(), w64)
    mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
    h_ref = F.relu((y - mean.view(1, -1, 1, 1)) * (var.view(1, -1, 1, 1) + bn.eps).rsqrt() * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1))
    (h_ref * probe.double()).sum().backward()
    n_px = N * H * W
    run_mean, run_var = 0.1 * mean.detach(), 0.9 + 0.1 * var.detach() * n_px / (n_px - 1)

    blk = blk.to(DEV).train()
    conv, bn = blk.net[0].conv, blk.net[1]
    calls, real = [], L.call
    L.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        t = E.Tape(True, DEV)
        xa = E.Act.empty(N, H, W, cin, DEV, zero=True)
        xa.data[..., :cin].copy_(x.to(DEV).permute(0, 2, 3, 1))
        out = E.conv_bn(t, E.tap_layer(conv), xa, bn, relu=True, need_input_grad=False)
        assert isinstance(out, E.Act)  # (the small-K path returns the activation itself, not a folded operand)
        t.set_grad(out, engine_bwd.grad_act_like(out, probe.to(DEV).to(torch.bfloat16)))
        t.backward()
        torch.cuda.synchronize()
    finally:
        L.call = real
    assert "rv_smallk_forward" in calls and any(c.startswith("rv_bn_bwd_smallk") for c in calls) and "rv_tap_gather" not in calls, calls
    assert rel_err(out.nchw().float().cpu(), h_ref.detach().float()) < 8e-3  # one bf16 store
    assert rel_err(bn.running_mean.cpu(), run_mean.float()) < 1e-3 and rel_err(bn.running_var.cpu(), run_var.float()) < 1e-3
    for name, p, ref in (("weight", conv.weight, w64.grad), ("gamma", bn.weight, gamma.grad), ("beta", bn.bias, beta.grad)):
        got = t.param_grads[id(p)].float().cpu()
        assert _cos(got, ref.float()) > 0.985 and rel_err(got, ref.float()) < 2e-2, (name, _cos(got, ref.float()), rel_err(got, ref.float()))


# ------------------------------------------------------------------------------------------------------------ repeatability screen
def test_repeatable_on_random_data():
    """Race screen (see test_gpu_tapconv4.py): fixed summation order => two launches on random data agree bit for bit -- the forward
    with the affine prologue at the full-size grid, and the split-K weight gradient of the same layer."""
    from range_view_3d_detection_amd import _lib as L

    g = torch.Generator().manual_seed(9)
    m = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False)
    m.weight.data = torch.randn(m.weight.shape, generator=g) * 0.05
    from range_view_3d_detection_amd import engine as E

    m = m.to(DEV)
    layer = E.tap_layer(m)
    x = _act(torch.randn(4, 64, 64, 2048, generator=g))
    dy = _act(torch.randn(4, 64, 64, 2048, generator=g))
    scale, shift = (0.5 + torch.rand(64, generator=g)).to(DEV), torch.randn(64, generator=g).to(DEV)
    flags = L.IN_AFFINE | L.IN_RELU
    first, p1, _ = _tap(layer, "gather", x, flags=flags, scale=scale, shift=shift, stats=True, expect=(2, 2))
    again, p2, _ = _tap(layer, "gather", x, flags=flags, scale=scale, shift=shift, stats=True, expect=(2, 2))
    assert torch.equal(first, again) and torch.equal(p1, p2)
    xin = F.relu(x.nchw().float().cpu()[:1, :, :6, :96] * scale.cpu().view(1, -1, 1, 1) + shift.cpu().view(1, -1, 1, 1)).bfloat16().float()
    ref = F.conv2d(xin, m.weight.data.cpu().bfloat16().float(), padding=1)[:, :, 1:5, 1:95]
    assert float((first[:1, :, 1:5, 1:95] - ref).abs().max()) / float(ref.abs().max()) < 1e-2  # bf16 output rounding
    w1, _ = _wgrad(layer.geom, 4, 64, 2048, dy, x, 2, flags=flags, scale=scale, shift=shift, v_affine=1)
    w2, _ = _wgrad(layer.geom, 4, 64, 2048, dy, x, 2, flags=flags, scale=scale, shift=shift, v_affine=1)
    assert torch.equal(w1, w2)
