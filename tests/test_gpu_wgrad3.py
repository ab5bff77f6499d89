"""The LDS-DMA weight-gradient kernel -- generation 3, ``wgrad3_kernel`` (csrc/wgrad.hip: 128 x 128 tiles of up to three taps of one
kernel row, 64-pixel chunks streamed into a ring of four LDS slots, split-K slabs + reduction) -- compared bit for bit with a reference
that does not touch this library: every split plan, tap group, image edge, operand stride and result layout, and the shapes the
models run at full size.

Method of test_gpu_tapconv2.py: operands in {-1, 0, 1}, so every partial sum is an integer below 2^24 (the largest case,
4 x 64 x 18432 = 4.7 M pixels, still is) and the result must EQUAL the reference whatever the split or the summation order.  The launches
go through the C ABI (``rv_tap_wgrad``).  Every case

* asserts ``rv_tap_wgrad_info(...)[0] == 3`` on the very shape it launches and, where a branch of the planner is the point of the case,
  the number of slabs and workgroups too (balanced split <=> workgroups != tiles x slabs), so that a change of the planner cannot
  silently move the case off the branch it is there for;
* starts from a NaN result and a NaN workspace: in the engine the workspace is recycled allocator memory that holds finite values, so a
  slab region that no workgroup writes is summed silently; with NaN it shows;
* names the taps, tiles and channel ranges that differ when it fails.

Reference: ``torch.nn.grad.conv2d_weight`` in fp32 on the CPU where that takes well under a second; above that
``_reference_on_device`` -- per tap the fp64 product U^T shift(V), image rows in blocks -- which
``test_device_reference_matches_the_cpu_function`` pins against the CPU function.
"""

from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_forward import DEV
from test_gpu_tapconv2 import _act, _wgrad
from test_gpu_tapconv4 import _ints

pytestmark = pytest.mark.gpu

NAN = float("nan")
CPU_REFERENCE_MAX_FLOP = 8e9  # above this the reference runs on the device


# ---------------------------------------------------------------------------------------------------------------- operands
def _operand(N, H, W, c, gen, half=None):
    """``engine.Act`` (N, H, W, c) of values in {-1, 0, 1}.  ``half`` = 0 / 1: the low / high half of a buffer twice as wide whose other half
    is NaN (pixel stride 2 c, on top of the kernel's own tile offsets): any read of the other half shows in the result."""
    from range_view_3d_detection_amd import engine as E

    x = torch.randint(-1, 2, (N, H, W, c), generator=gen, device=DEV, dtype=torch.bfloat16)
    if half is None:
        return E.Act(x)
    wide = torch.full((N, H, W, 2 * c), NAN, dtype=torch.bfloat16, device=DEV)
    wide[..., half * c:(half + 1) * c] = x
    return E.Act(wide).slice(half * c, (half + 1) * c)


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)))


# --------------------------------------------------------------------------------------------------------------- references
def _reference_on_cpu(u, v, kh, kw, ph, pw):
    """dT[cu][cv][ky][kx] = sum_{n,h,w} U[n,h,w,cu] V[n,h+ky-ph,w+kx-pw,cv] (zero outside the image) as the weight gradient of the
    stride-1 convolution of the explicitly padded V; ``u`` / ``v``: (N, H, W, C) views."""
    x = F.pad(v.permute(0, 3, 1, 2).float().cpu().contiguous(), (pw, kw - 1 - pw, ph, kh - 1 - ph))
    dy = u.permute(0, 3, 1, 2).float().cpu().contiguous()
    return torch.nn.grad.conv2d_weight(x, (u.shape[3], v.shape[3], kh, kw), dy)


def _reference_on_device(u, v, kh, kw, ph, pw, block_elems=1 << 27):
    """The same sum written out: per image and block of rows, U as (rows, cu, W) and the zero-framed V as (rows + kh - 1, W + kw - 1, cv) in
    fp64; tap (ky, kx) is the batched product of U with the frame shifted by (ky, kx), summed over the rows.  Integer data: exact."""
    N, H, W, cu = u.shape
    cv = v.shape[3]
    out = torch.zeros((kh, kw, cu, cv), dtype=torch.float64, device=u.device)
    rows = max(1, min(H, block_elems // (W * max(cu, cv))))
    for n in range(N):
        for h0 in range(0, H, rows):
            h1 = min(H, h0 + rows)
            ub = u[n, h0:h1].double().transpose(1, 2)
            frame = torch.zeros((h1 - h0 + kh - 1, W + kw - 1, cv), dtype=torch.float64, device=u.device)  # row j = image row h0 - ph + j
            lo, hi = max(0, h0 - ph), min(H, h1 + kh - 1 - ph)
            frame[lo - (h0 - ph):hi - (h0 - ph), pw:pw + W] = v[n, lo:hi].double()
            for ky in range(kh):
                for kx in range(kw):
                    out[ky, kx] += torch.bmm(ub, frame[ky:ky + h1 - h0, kx:kx + W]).sum(dim=0)
    assert float(out.abs().max()) < 2 ** 24
    return out.permute(2, 3, 0, 1).float().cpu().contiguous()


def _reference(u, v, kh, kw, ph, pw):
    N, H, W, cu = u.shape
    flop = 2.0 * N * H * W * kh * kw * cu * v.shape[3]
    return (_reference_on_cpu if flop <= CPU_REFERENCE_MAX_FLOP else _reference_on_device)(u, v, kh, kw, ph, pw)


def _assert_exact(got, ref, what):
    """``got == ref`` element for element (cu, cv, kh, kw); the message says where they differ: taps, 128 x 128 tiles, channel ranges."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = got != ref  # (NaN differs from everything)
    idx = bad.nonzero()
    taps = sorted(set(map(tuple, idx[:, 2:].tolist())))
    tiles = sorted(set(map(tuple, (idx[:, :2] // 128).tolist())))
    first = [(tuple(i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx[:6].tolist()]
    raise AssertionError(
        f"{what}: {len(idx)} of {bad.numel()} entries differ ({int(got.isnan().sum())} NaN); taps (ky, kx) {taps}; tiles (cu / 128, cv / 128) {tiles}; "
        f"cu {int(idx[:, 0].min())}..{int(idx[:, 0].max())}, cv {int(idx[:, 1].min())}..{int(idx[:, 1].max())}; "
        f"largest difference {float((got - ref).nan_to_num(0.0).abs().max())}; first (index, got, reference): {first}")


# ------------------------------------------------------------------------------------------------------------------ the case
def _geom(kh, kw, ph, pw, cu, cv):
    from range_view_3d_detection_amd import _lib as L

    return L.TapGeom(kh, kw, 1, ph, pw, cu, cv)


def _tiles(g):
    return g.kh * ((g.kw + 2) // 3) * ((g.cu + 127) // 128) * ((g.cv + 127) // 128)  # tap groups x channel tiles


def _check_plan(g, info, plan, what):
    """``plan`` = (slabs, workgroups, balanced) or None."""
    if plan is None:
        return
    slabs, workgroups, balanced = plan
    assert info[1:3] == [slabs, workgroups], (what, info)
    assert (info[2] != _tiles(g) * info[1]) == balanced, (what, info, _tiles(g))


def _exact_case(kernel, cu, cv, N, H, W, plan=None, halves=(None, None), torch_layout=True):
    kh, kw, ph, pw = kernel
    what = f"{kh}x{kw} pad ({ph}, {pw}), {cu} <-> {cv}, {N} x {H} x {W}"
    g = _geom(kh, kw, ph, pw, cu, cv)
    gen = _gen(kh, kw, cu, cv, N, H, W)
    u = _operand(N, H, W, cu, gen, halves[0])
    v = _operand(N, H, W, cv, gen, halves[1])
    got, info = _wgrad(g, N, H, W, u, v, 3, torch_layout=torch_layout, nan_workspace=True)
    _check_plan(g, info, plan, what)
    _assert_exact(got, _reference(u.data, v.data, kh, kw, ph, pw), f"{what}, plan {info[:3]}")
    return info


K1, K3 = (1, 1, 0, 0), (3, 3, 1, 1)
K3x1, K1x3, K3x2, K3x4, K3x8 = (3, 1, 1, 0), (1, 3, 0, 1), (3, 2, 1, 1), (3, 4, 1, 1), (3, 8, 1, 2)


def test_device_reference_matches_the_cpu_function():
    """``_reference_on_device`` against ``torch.nn.grad.conv2d_weight`` on the CPU: the widest kernel (eight columns, uneven padding), two
    channel counts, V a slice of a wider buffer, and row blocks that end inside an image (17 rows in blocks of 3)."""
    N, H, W, cu, cv = 2, 17, 150, 128, 64
    gen = _gen(N, H, W)
    u, v = _operand(N, H, W, cu, gen), _operand(N, H, W, cv, gen, half=1)
    for kernel in (K3x8, K3, K1):
        ref = _reference_on_cpu(u.data, v.data, *kernel)
        assert ref.abs().max() > 16  # not a comparison of zeros
        _assert_exact(_reference_on_device(u.data, v.data, *kernel, block_elems=3 * W * cu), ref, f"device reference, kernel {kernel}")


# -------------------------------------------------------------------------------------------------------------- a. split plans
@pytest.mark.parametrize("kernel,cu,cv,N,H,W,plan", [
    # slices shorter than the ring of four: the prologue's second and third chunk lie past the slice and come from the zero page, with the
    # same instruction count (the waits are counted); three workgroups: the XCD remap with a remainder
    pytest.param(K3, 128, 128, 1, 1, 64, (1, 3, False), id="1-chunk-shorter-than-the-ring"),
    pytest.param(K3, 128, 128, 2, 1, 64, (1, 3, False), id="2-chunks-shorter-than-the-ring"),
    pytest.param(K3, 128, 128, 1, 5, 64, (1, 3, False), id="5-chunks"),
    pytest.param(K3, 128, 128, 2, 3, 100, (1, 3, False), id="12-chunks-grid-of-3"),
    # the four exits of the K loop (it is unrolled over the four ring slots): chunks per slice = 4n, 4n + 1, 4n + 2, 4n + 3
    pytest.param(K3, 128, 128, 2, 2, 166, (1, 3, False), id="loop-exit-4n-12-chunks"),
    pytest.param(K3, 128, 128, 3, 1, 166, (1, 3, False), id="loop-exit-4n+1-9-chunks"),
    pytest.param(K3, 128, 128, 2, 3, 166, (1, 3, False), id="loop-exit-4n+2-18-chunks"),
    pytest.param(K3, 128, 128, 3, 3, 166, (1, 3, False), id="loop-exit-4n+3-27-chunks"),
    # 306 chunks = 9 slices of 34, six chunks per image row: the slices begin in the middle of a row, the last chunk of a row has 13 pixels
    pytest.param(K3, 128, 128, 3, 17, 333, (9, 27, False), id="slices-begin-mid-row-9x34"),
    # balanced split: five regular slices per tile + 16 remainder workgroups that finish three tiles each into a sixth slab (ragged rows;
    # the smallest shape that reaches it -- at W = 128 the same layer takes the plain 5 x 48)
    pytest.param(K3, 512, 512, 4, 64, 166, (6, 256, True), id="balanced-3-tiles-per-remainder-workgroup"),
    pytest.param(K3, 512, 512, 4, 64, 128, (5, 240, False), id="plain-5x48"),
    # 45 tiles, 23 remainder workgroups of two: the last one has ONE tile (no shipped model reaches this, the ABI does)
    pytest.param(K3, 384, 640, 4, 64, 512, (6, 248, True), id="balanced-last-remainder-workgroup-has-1-tile"),
    # the longest remainder loop the planner allows: four tiles in turn (the ring rewritten three times)
    pytest.param(K3, 512, 640, 4, 64, 512, (5, 255, True), id="balanced-4-tiles-per-remainder-workgroup"),
    pytest.param(K1, 640, 896, 4, 64, 512, (8, 254, True), id="balanced-4-tiles-1x1-last-has-3"),
    # 54 tiles in six tap groups of nine, remainder workgroups of two: every ninth one finishes a tile of a three-tap group and then a
    # tile of a one-tap group (``wgrad3_body<3>`` and ``<1>`` in turn on the same ring)
    pytest.param(K3x4, 384, 384, 4, 64, 512, (5, 243, True), id="balanced-remainder-workgroup-spans-a-3-tap-and-a-1-tap-group"),
    pytest.param(K3x8, 128, 128, 3, 17, 333, (9, 81, False), id="slices-begin-mid-row-groups-of-3+3+2"),
    pytest.param(K3, 256, 256, 4, 64, 512, (21, 252, False), id="plain-21x12"),
    pytest.param(K1, 128, 128, 4, 64, 512, (64, 64, False), id="plain-1-tile-64-workgroups"),
])
def test_split_plans(kernel, cu, cv, N, H, W, plan):
    _exact_case(kernel, cu, cv, N, H, W, plan=plan)


# --------------------------------------------------------------------------------------------------------------- b. tap groups
@pytest.mark.parametrize("kernel,cu,cv,N,H,W", [
    pytest.param(K1, 128, 256, 3, 9, 200, id="1x1-one-group-of-1"),
    pytest.param(K3, 256, 128, 2, 5, 166, id="3x3-three-groups-of-3"),
    pytest.param(K3x1, 128, 128, 3, 4, 130, id="3x1-three-groups-of-1"),
    pytest.param(K1x3, 128, 256, 2, 6, 333, id="1x3-one-group-of-3"),
    pytest.param(K3x2, 128, 256, 2, 5, 166, id="3x2-groups-of-2"),               # the folded stride-2 3x3
    pytest.param(K3x4, 128, 128, 3, 7, 200, id="3x4-groups-of-3+1-dw0--1,2"),
    pytest.param(K3x8, 256, 128, 2, 9, 333, id="3x8-groups-of-3+3+2-dw0--2,1,4"),
])
def test_tap_groups(kernel, cu, cv, N, H, W):
    """One, two and three taps per group (``wgrad3_body<1|2|3>``: the halo rows 64 .. 64 + taps - 2), several groups per kernel row
    with first columns -2, 1, 4, and cu != cv (a tile index taken for the other operand's shows)."""
    _exact_case(kernel, cu, cv, N, H, W)


@pytest.mark.parametrize("kind,kernel,stride,pad,folded_kw", [
    pytest.param("conv", (3, 3), 2, (1, 1), 2, id="conv-3x3-stride-2"),
    pytest.param("conv", (1, 1), 2, (0, 0), 1, id="conv-1x1-stride-2"),
    pytest.param("convT", (3, 4), 2, (1, 1), 3, id="conv-transpose-3x4-stride-2"),
    pytest.param("convT", (3, 8), 4, (1, 2), 3, id="conv-transpose-3x8-stride-4"),
])
def test_strided_layers_through_the_folded_view(kind, kernel, stride, pad, folded_kw):
    """The strided layers as the engine runs them: ``rv_fold_geom`` -> generation 3 on the stride-1 view of the fine tensor (pixel stride
    ``stride * ld``, ``stride * 128`` channels) -> ``rv_unfold_weight_grad``, exact against the STRIDED torch operation."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    N, H, Wu, c = 2, 5, 166, 128
    g = torch.Generator().manual_seed(kernel[1] + stride)
    coarse, fine = _ints((N, c, H, Wu), g, -1, 2), _ints((N, c, H, Wu * stride), g, -1, 2)
    if kind == "conv":
        m = torch.nn.Conv2d(c, c, kernel, stride=(1, stride), padding=pad, bias=False).to(DEV)
        ref = torch.nn.grad.conv2d_weight(fine, m.weight.shape, coarse, stride=(1, stride), padding=pad)
    else:
        m = torch.nn.ConvTranspose2d(c, c, kernel, stride=(1, stride), padding=pad, bias=False).to(DEV)
        w = torch.zeros(m.weight.shape, requires_grad=True)
        (F.conv_transpose2d(coarse, w, stride=(1, stride), padding=pad) * fine).sum().backward()
        ref = w.grad
    layer = E.tap_layer(m)
    gf = layer.fold_geom()
    assert (gf.kh, gf.kw, gf.stride_w, gf.cu, gf.cv) == (kernel[0], folded_kw, 1, c, stride * c)
    u, v = _act(coarse), _act(fine)
    folded, _ = _wgrad(gf, N, H, Wu, u, v, 3, ld_v=stride * v.ld, nan_workspace=True)
    folded = folded.to(DEV)
    got = torch.full(tuple(m.weight.shape), NAN, dtype=torch.float32, device=DEV)
    L.call("rv_unfold_weight_grad", ctypes.byref(layer.geom), L.ptr(folded), L.ptr(got), 0, L.stream_ptr())
    torch.cuda.synchronize()
    _assert_exact(got.cpu(), ref, f"{kind} {kernel} stride {stride}")


# -------------------------------------------------------------------------------------------------------------- c. image edges
@pytest.mark.parametrize("N,H,W", [
    pytest.param(2, 1, 64, id="H1-W64-every-chunk-first-and-last-of-its-row"),
    pytest.param(3, 1, 333, id="H1-W333"),
    pytest.param(2, 2, 65, id="H2-W65-last-chunk-1-pixel"),
    pytest.param(3, 3, 127, id="W127"),
    pytest.param(2, 2, 128, id="H2-W128"),
    pytest.param(2, 5, 166, id="W166"),
    pytest.param(2, 3, 1808, id="W1808-28-chunks+16"),
    pytest.param(2, 2, 2656, id="H2-W2656-41-chunks+32"),
])
@pytest.mark.parametrize("kernel", [pytest.param(K3, id="3x3"), pytest.param(K3x8, id="3x8")])
def test_image_edges(kernel, N, H, W):
    """Row and image edges (the zero page takes the place of what lies outside): with H = 1 two of the three tap rows are outside the image
    for every chunk; N >= 2, so a tap row taken from the neighbouring image of the batch changes the result; the eight-column kernel
    reaches two pixels to the left and five to the right of the chunk."""
    _exact_case(kernel, 128, 128, N, H, W)


# --------------------------------------------------------------------------------------------------------- d. strided operands
@pytest.mark.parametrize("c,halves,N,H,W", [
    pytest.param(128, (0, 1), 3, 17, 333, id="128-U-low-V-high"),
    pytest.param(128, (1, 0), 3, 17, 333, id="128-U-high-V-low"),
    pytest.param(256, (1, 1), 2, 5, 166, id="256-both-high-two-tiles-each"),
    pytest.param(256, (0, None), 2, 5, 166, id="256-U-low-V-plain"),
])
def test_operands_that_are_halves_of_wider_buffers(c, halves, N, H, W):
    """``ld_u`` / ``ld_v`` twice the channel count (with the tile offsets on top); the other half of each buffer is NaN.  (Pixel stride
    ``stride * ld`` on V, as the folded view passes it: ``test_strided_layers_through_the_folded_view``.)"""
    _exact_case(K3, c, c, N, H, W, halves=halves)


# ----------------------------------------------------------------------------------------------------------- e. result layouts
@pytest.mark.parametrize("torch_layout", [pytest.param(True, id="torch-layout"), pytest.param(False, id="packed-tap-cu-cv")])
def test_result_layouts(torch_layout):
    """``RV_WGRAD_TORCH_LAYOUT`` (dT[cu][cv][kh][kw], written by the reduction) and the packed [tap][cu][cv] form on a shape with six channel
    tiles, three tap groups and five slabs."""
    info = _exact_case(K3, 256, 384, 2, 9, 600, torch_layout=torch_layout)
    assert info[1] > 1, info


# -------------------------------------------------------------------------------------------------- f. the shapes the models run
@pytest.mark.parametrize("kernel,cu,cv,N,H,W,plan", [
    pytest.param(K3, 512, 512, 4, 64, 2048, (6, 256, True), id="3x3-512-W2048-balanced"),
    pytest.param(K3, 256, 256, 4, 64, 2048, (21, 252, False), id="3x3-256-W2048"),
    pytest.param(K3, 256, 256, 4, 64, 2656, (21, 252, False), id="3x3-256-W2656"),
    pytest.param(K3, 128, 128, 4, 64, 2656, (85, 255, False), id="3x3-128-W2656"),
    pytest.param(K1, 256, 2304, 4, 64, 2048, (7, 252, False), id="1x1-256-2304-W2048-36-tiles"),
    pytest.param(K1, 128, 128, 4, 64, 2656, (256, 256, False), id="1x1-128-W2656-1-tile-256-slices"),
    # the MetaKernel fusion conv's nine-tap operand as one 1x1 layer: 2.4 GB per operand, every pixel offset beyond 2^31 bytes from the middle
    # of the tensor on -- the only place where a 32-bit offset would show
    pytest.param(K1, 256, 256, 4, 64, 18432, (64, 256, False), id="1x1-256-W18432-offsets-beyond-2^31"),
])
def test_model_shapes_at_full_size(kernel, cu, cv, N, H, W, plan):
    _exact_case(kernel, cu, cv, N, H, W, plan=plan)


# ------------------------------------------------------------------------------------------- g. bit-identity with generation 2
@pytest.mark.parametrize("kernel,cu,cv,N,H,W", [
    pytest.param(K3, 256, 128, 3, 17, 333, id="3x3-256-128-ragged"),
    pytest.param(K1, 128, 256, 2, 64, 512, id="1x1-128-256"),
    pytest.param(K3, 128, 128, 4, 64, 2656, id="3x3-128-W2656-85-slabs"),
])
def test_bit_identical_to_generation_2_on_random_data(kernel, cu, cv, N, H, W):
    """Random bf16 operands, the same layer on both generations with the same split: generation 3 plainly, generation 2 by asking for the
    folded-BatchNorm prologue with scale 1 and shift 0 (not eligible for the DMA kernel).  Both feed the same pixels to the same MFMA
    sequence per accumulator and the reduction adds the same slabs in the same order, so the results are equal bit for bit."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    g = _geom(*kernel, cu, cv)
    gen = _gen(*kernel, cu, cv, N, H, W)
    u = E.Act(torch.randn((N, H, W, cu), generator=gen, device=DEV).bfloat16())
    v = E.Act(torch.randn((N, H, W, cv), generator=gen, device=DEV).bfloat16())
    got3, info3 = _wgrad(g, N, H, W, u, v, 3, nan_workspace=True)
    got2, info2 = _wgrad(g, N, H, W, u, v, 2, flags=L.IN_AFFINE, scale=torch.ones(cv, device=DEV), shift=torch.zeros(cv, device=DEV), v_affine=1,
                         nan_workspace=True)
    assert info3[1:3] == info2[1:3] and info3[1] > 1, (info3, info2)  # the same slices on both
    assert got3.isfinite().all() and float(got3.abs().max()) > 1.0
    _assert_exact(got3, got2, f"generation 3 against generation 2, {kernel} {cu} <-> {cv}, {N} x {H} x {W}")
