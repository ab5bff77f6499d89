"""The fp16 inference build (``librv3d_hip_f16.so``) at fp16's OWN edges, and eval-mode BatchNorm scales away from 1 on both builds.

The kernel-level fp16 tests elsewhere reuse the bf16 tests' small integers, which fp16 holds exactly: nothing there rounds, underflows
or overflows.  Here the data are sized for fp16.  Method of test_gpu_stem_kernels.py: the reference is the exact fp64 result
(``fp16_ref.py``), cast once to fp16 by torch's CPU cast (round to nearest even, gradual underflow, infinity from 65520 on); the
preconditions -- every partial sum exact in fp32 whatever the order, and the shares of outputs that round / underflow / overflow -- are
asserted from the data alone before any launch; every output is pre-filled with SENTINEL and has a spare image behind it that must stay
untouched; every launch asserts its kernel generation from ``rv_tap_launch_info``.  Comparison: ``torch.equal`` (infinities equal
infinities, a NaN equals nothing).

1. ROUNDING past 11 bits: non-negative integers, sums around 2048 in half of the output channels (weights in {0, 1}) and around 4096 in
   the other half (weights in {0, 1, 2}): ties and non-ties; a truncating or twice-rounding store fails.  Fold: gamma in {0.5, 1, 2}.
2. SUBNORMALS: (a) a weight image of fp16 subnormals (integer weights under a fold of 2^-22; on generation 7, which takes no bias, the
   same values as a plain image) against activations k x 2^8; (b) subnormal activations k x 2^-24 whose sums are stored as subnormals.
3. OVERFLOW: fold 16 on sums around 4032: 65504 (largest finite) and 65520 (tie: +inf) both occur; -inf under ReLU stores 0; inf plus a
   finite residual stays inf (the conv result is rounded to fp16 BEFORE the residual is added: rv_tap_residual's contract).
4. BATCHNORM SCALES over many decades (both builds, random data): the fold contract of ``fp16_ref.fold_emulation`` within a derived
   per-element bound, and per channel no further from fp64 BatchNorm than twice what the reference's unfolded route is.  Where the
   fp16 image of the folded weights would underflow, the engine must not fold (``TapLayer.eval_fold_ok``): asserted, with the same two
   checks on the route it takes instead.
5. RESCALED TWIN of the tiny detector (both builds, EVAL_FOLD on and off): see test_rescaled_twin.

Kernel form an eval program launches in the fp16 build -> the case that rounds past 11 bits / the subnormal cases / the overflow case
(plain = ConvOp, fold = conv_bn, res = conv_bn_residual with either ReLU placement):

* tapconv5<256> 3x3 ............ test_rounding[3x3-gen5-*] / test_subnormal[3x3-gen5-*] / test_overflow[3x3-gen5-*]
* tapconv6 3x3 ................. test_rounding[3x3-gen6-*] / test_subnormal[3x3-gen6-*] / test_overflow[3x3-gen6-*]
* tapconv4<256> 1x1 ............ test_rounding[1x1-*], [1x1p-*-fold|res_*] / test_subnormal[1x1-*] / test_overflow[1x1p-*] (fold, neg, res)
* pointwise GEMM (7) ........... test_rounding[1x1p-*-plain] / test_subnormal[1x1p-*] (plain images) / none: it takes no bias, so no fold
  reaches it, and a plain conv of fp16 operands that overflows is the same store as the rounding case
* folded stride-(1,2) 3x3 ...... test_rounding[3x3s2-gen5|gen6-*] / none, none: the same tapconv5 / tapconv6 kernels and epilogues as the 3x3
  rows above, on the folded view -- what differs is the tap table, which the rounding case covers
* conv-transpose phases ........ test_rounding[convT-gen5|gen6-*] / none, none: as the row above (the scatter form's phase loop)
* generic (register-staged) .... test_rounding[3x3g-*], [1x1g-*] / test_subnormal[3x3g-*], [1x1g-*] / none: its store is the shared
  epilogue function the rounding case pins, the overflow being a property of that one conversion
* rv_ew_combine ................ test_combine_rounding / none: no eval program feeds it anything but stored activations; sums of two
  subnormal or two huge activations go through the same ``f2bf`` as the rounding case

FOUND by these tests (MI355X): items 1, 2, 3 and 5 passed as first written -- every store rounds to nearest even once, subnormal fp16
operands go through ``v_mfma_f32_16x16x32_f16`` and the generic kernels unflushed, subnormal results are stored unflushed, 65520 becomes
+inf, -inf under ReLU stores 0.  Item 4 failed in the fp16 build with every layer folded: with scales of 2^-10 and below the folded
weights are fp16 subnormals (24 % of the "gamma" image), held to an absolute 2^-24, and those channels were up to 7.5 x further from
fp64 BatchNorm than the reference's route (3x3 "gamma": fold max 2.67e-03 of the channel maximum against 7.73e-04, worst ratio 7.52;
1x1: 3.83e-03 against 1.25e-03, 6.81; "var", scales down to 2^-10: 1.74 and 1.49, inside the factor two) while every element stayed
inside the contract's bound: the kernels were right, the image was too coarse.  The engine now leaves such a layer unfolded.

Figures of the run after that change, per channel of its own maximum against fp64 BatchNorm (fold or fallback route: median, max /
the reference's unfolded route: median, max / worst per-channel ratio; generations 5 and 6 give the same numbers):

* 3x3 var   f16 (fallback) 4.94e-04 8.07e-04 / 4.94e-04 8.07e-04 / 1.00      bf16 (fold) 2.86e-03 4.03e-03 / 3.83e-03 6.96e-03 / 1.09
* 3x3 gamma f16 (fallback) 4.76e-04 7.73e-04 / 4.76e-04 7.73e-04 / 1.00      bf16 (fold) 2.84e-03 4.38e-03 / 3.98e-03 7.61e-03 / 1.11
* 3x3 mid   f16 (fold)     3.59e-04 5.28e-04 / 4.81e-04 8.17e-04 / 1.31      bf16 (fold) 2.85e-03 4.07e-03 / 3.87e-03 7.14e-03 / 1.10
* 1x1 var   f16 (fallback) 5.20e-04 8.96e-04 / 5.20e-04 8.96e-04 / 1.00      bf16 (fold) 3.03e-03 4.74e-03 / 4.15e-03 7.78e-03 / 1.29
* 1x1 gamma f16 (fallback) 5.15e-04 1.25e-03 / 5.15e-04 1.25e-03 / 1.00      bf16 (fold) 3.05e-03 4.70e-03 / 4.14e-03 9.32e-03 / 1.14
* 1x1 mid   f16 (fold)     3.82e-04 5.67e-04 / 5.41e-04 8.26e-04 / 1.27      bf16 (fold) 3.11e-03 4.30e-03 / 4.13e-03 7.14e-03 / 1.39

(The fallback route equals the emulation of the reference's route bit for bit, hence 1.00.)  Rescaled twin, 1376 channels: fp16 folded
j < 0 on 21 %, j > 0 on 60 %, |j| >= 4 on 40 %; fp16 unfolded 0 / 79 / 46 %; bf16 52 / 43 / 60 %: logits and regressands equal in all four.
"""

from __future__ import annotations

import contextlib

import pytest
import torch

import bn_ref as BR
import fp16_ref as R
from test_gpu_bn_passes import SENTINEL, _Data, _info, _Out
from test_gpu_forward import DEV
from test_gpu_tapconv4 import _ints

pytestmark = pytest.mark.gpu

F16 = torch.float16
GENERIC = 1
# (route, the generation the SEL_* hints admit for halo-resident layers) -> the generation of the plain / the folded and residual forms
ROUTE_GENS = {("3x3", 5): (5, 5), ("3x3", 6): (6, 6), ("1x1", 5): (4, 4), ("1x1p", 5): (7, 4), ("3x3s2", 5): (5, 5), ("3x3s2", 6): (6, 6),
              ("convT", 5): (5, 5), ("convT", 6): (6, 6), ("3x3g", 5): (GENERIC, GENERIC), ("1x1g", 5): (GENERIC, GENERIC)}
ALL_ROUTES = sorted(ROUTE_GENS)
EDGE_ROUTES = [k for k in ALL_ROUTES if k[0] in R.SUB_ROUTES]
_id = lambda k: f"{k[0]}-gen{k[1]}"


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    R.release_cases()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _small_grids_allowed(gen):
    """Crops this small stay below the libraries' tile-count thresholds: lift them, with the halo-resident layers on the fifth
    generation or on the sixth (the fixture of test_gpu_evalfold.py, by argument)."""
    from range_view_3d_detection_amd import _lib as L

    with L.select(L.SEL_SMALL_GRIDS | (L.SEL_SMALL_GRIDS6 if gen == 6 else L.SEL_NO_GEN6)):
        yield


def _module(r, w):
    from range_view_3d_detection_amd.nn.modules.conv import Conv2dSame

    if r.kind == "convT":
        m = torch.nn.ConvTranspose2d(r.cin, r.cout, kernel_size=(3, 4), stride=(1, 2), padding=(1, 1), bias=False)
    else:
        m = Conv2dSame(r.cin, r.cout, r.k, stride=(1, r.stride_w), bias=False).conv
    assert m.weight.shape == w.shape
    m.weight.data = w.clone()
    return m.to(DEV)


def _bn(c, gamma, beta=None, mean=None, var=None):
    bn = torch.nn.BatchNorm2d(c, eps=0.0)
    zero = torch.zeros(c)
    bn.weight.data, bn.bias.data = gamma.float().clone(), (zero if beta is None else beta).float().clone()
    bn.running_mean.data, bn.running_var.data = (zero if mean is None else mean).float().clone(), (torch.ones(c) if var is None else var).float().clone()
    return bn.eval().to(DEV)


def _planned(E, L, layer, op):
    """rv_tap_launch_info of the launch ``op`` made: on the folded stride-1 view where the engine took that (asserted from the image it
    packed), on the layer's own geometry otherwise."""
    geom, shape = layer.geom, op.shape
    if layer.geom.stride_w > 1 and layer.fwd_form == "gather":
        slot = E.image_slot("folded", "eval_fold" if op.eval_bn is not None else None)
        assert layer.images.held(slot) is not None, "the strided layer did not run on its folded view"
        geom = layer.fold_geom()
        shape = L.TapShape(shape.N, shape.H, shape.Wu, shape.Wu, layer.geom.stride_w * shape.ld_src, shape.ld_dst, shape.flags)
    info = L.tap_launch_info(geom, shape, layer.fwd_form == "scatter")
    assert info is not None, L.load().rv_last_error()
    return info


def _launch(r, gen, expect, x, module, bn=None, relu=True, res=None, res_relus=None, tag="f16"):
    """One tap op on route ``r``: plain (``bn`` None), folded BatchNorm (+ ReLU), or folded BatchNorm + residual.  The operands are cast
    to the operand type on the CPU (exact for the exact cases) and the output is a sentinel-filled buffer with a spare image behind."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    dt = F16 if tag == "f16" else torch.bfloat16
    to_dev = lambda t: t.to(dt).to(DEV)
    assert torch.equal(x.to(dt).float(), x.float()), "the activations are not exact in the operand type"
    with _small_grids_allowed(gen), L.operand(tag):
        t = E.Tape(False, DEV)
        layer = E.tap_layer(module)
        xa = E.Act.from_nchw(to_dev(x))
        buf = torch.full((r.N + 1, r.H, r.w_out, r.cout), SENTINEL, dtype=dt, device=DEV)
        out = E.Act(buf[: r.N])
        if bn is None:
            y = E.ConvOp(t, layer, xa, out=out).out
        elif res is None:
            y = E.conv_bn(t, layer, xa, bn, relu=relu, out=out)
        else:
            y = E.conv_bn_residual(t, layer, xa, bn, E.Act.from_nchw(to_dev(res)), *res_relus, out=out)
        assert y is out and len(t.ops) == 1  # one launch, writing where it was told
        info = _planned(E, L, layer, t.ops[0])
        assert info[0] == expect, (info, expect)
        torch.cuda.synchronize()
    assert bool((buf[r.N] == SENTINEL).all()), "wrote behind its last image"
    return out.nchw().cpu()


def _assert_bits(got, exact, what):
    """got equals the exact fp64 value rounded once to fp16, bit pattern for bit pattern (inf = inf, no NaN)."""
    want = R.to16(exact)
    assert not bool(got.isnan().any()), f"{what}: NaN stored"
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)]), float(exact[tuple(i)])) for i in bad[:6]]
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; channels {sorted(set(bad[:, 1].tolist()))[:16]}; "
                         f"first (index, got, want, exact): {first}")


# ------------------------------------------------------------------------------------------------------------------ 1. rounding
@pytest.mark.parametrize("form", ["plain", "fold", "res_out", "res_conv"])
@pytest.mark.parametrize("key", ALL_ROUTES, ids=_id)
def test_rounding(key, form):
    name, gen = key
    c = R.rounding_case(name, _ints)
    r, exact = c["route"], c["exact"][form]
    # from the data alone: fp32 accumulation is exact, and the stores round -- ties and non-ties, above and below 2048
    if form == "plain":
        R.assert_exact_in_fp32(r, c["x"], c["w"], None, 1.0, 1.0)
    else:
        R.assert_exact_in_fp32(r, c["x"], c["wf"], c["shift"], 1.0, 0.5)
        R.assert_rounding_shares(c["exact"]["fold"], c["wide"], f"{name} the conv result under the residual")
    R.assert_rounding_shares(exact, c["wide"], f"{name} {form}")
    expect = ROUTE_GENS[key][0 if form == "plain" else 1]
    m = _module(r, c["w"])
    if form == "plain":
        got = _launch(r, gen, expect, c["x"], m)
    else:
        bn = _bn(r.cout, c["gamma"], c["beta"], c["mean"])
        got = _launch(r, gen, expect, c["x"], m, bn, res=None if form == "fold" else c["res"], res_relus=R.RES_FORMS.get(form))
    _assert_bits(got, exact, f"{name} gen{gen} {form}")


def test_combine_rounding():
    """rv_ew_combine in the fp16 build at 999 x 96 (the shape of test_fp16_build_combine) with operands up to 2047 (a) and 4094 (b, even) and scales in
    {1, 2}: the sums reach past 2048 and 4096 -- exact in fp32, rounded once by the store."""
    from range_view_3d_detection_amd import _lib as L

    n, c = 999, 96
    with L.operand("f16"):
        D = _Data(n, c, seed=4242, dtype=F16)
        g = torch.Generator(device=DEV).manual_seed(4243)
        D.y = torch.randint(0, 2048, (n, c), generator=g, device=DEV).to(F16)
        D.yb = (2 * torch.randint(0, 2048, (n, c), generator=g, device=DEV)).to(F16)  # (even, up to 4094: a + b alone passes 4096)
        for i, (has_b, aff_a, aff_b, flags) in enumerate([(True, True, True, BR.EW_RELU_OUT), (True, False, False, 0), (True, True, False, BR.EW_RELU_A | BR.EW_RELU_B)]):
            layout = ("dense", "pitched", "offset")[i]
            (a, ld_a), (b, ld_b) = D.op("y", layout, n), D.op("yb", layout, n)
            sa, ta = (D.sa, D.ta) if aff_a else (None, None)
            sb, tb = (D.sb, D.tb) if aff_b else (None, None)
            exact = BR.combine(D.y, sa, ta, D.yb, sb, tb, flags).cpu()
            s = R.shares(exact)
            assert s["above"] >= 0.2 and s["below"] >= 0.1 and s["ties"] >= 0.05 and s["nonties"] >= 0.05 and float(exact.abs().max()) < 1 << 14, s
            o = _Out(n, c, F16)
            assert _info(L.EW_PASS_COMBINE, n, c, None, has_b)[:3] == (L.EW_FORM_COMB, 0, (n * (c // 8) + 255) // 256)
            L.call("rv_ew_combine", n, c, L.ptr(a), ld_a, L.ptr(sa), L.ptr(ta), L.ptr(b), ld_b, L.ptr(sb), L.ptr(tb), L.ptr(o.view), o.ld, flags, L.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(o.view.cpu(), R.to16(exact)), (layout, int((o.view.cpu() != R.to16(exact)).sum()))
            assert bool((o.buf[:, :8] == SENTINEL).all()) and bool((o.buf[:, 8 + c:] == SENTINEL).all()) and bool((o.buf[n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------ 2. subnormals
@pytest.mark.parametrize("which", ["weights", "acts"])
@pytest.mark.parametrize("key", EDGE_ROUTES, ids=_id)
def test_subnormal(key, which):
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    name, gen = key
    c = R.subnormal_case(name, which, _ints)
    r, exact = c["route"], c["exact"]
    R.assert_exact_in_fp32(r, c["x"], c["wf"], None, c["ux"], c["uw"])
    assert torch.equal(R.to16(exact).double(), exact)  # every output is a value fp16 holds (subnormals included)
    s = R.shares(exact)
    sub = lambda t: (t != 0) & (t.abs() < R.F16_MIN_NORMAL)
    if which == "acts":
        assert s["subnormal"] >= 0.95 and bool(sub(c["x"]).sum() >= 0.8 * c["x"].numel()), s  # subnormal in, subnormal out
        got = _launch(r, gen, ROUTE_GENS[key][0], c["x"], _module(r, c["w"]))
    else:
        assert bool(sub(c["wf"]).sum() >= 0.8 * c["wf"].numel()) and float((exact != 0).sum()) >= 0.99 * exact.numel()
        assert float(exact.abs().max()) < 2048 * R.F16_MIN_NORMAL and float(exact.abs().max()) > 256 * R.F16_MIN_NORMAL
        folded_form = ROUTE_GENS[key][0] != 7
        if folded_form:
            m, bn = _module(r, c["w"]), _bn(r.cout, torch.full((r.cout,), R.SUB_GAMMA))
            got = _launch(r, gen, ROUTE_GENS[key][1], c["x"], m, bn, relu=False)
        else:  # (generation 7 takes no bias: the subnormal values reach it as a plain image)
            m = _module(r, c["wf"])
            got = _launch(r, gen, 7, c["x"], m)
        # the weight image, read back: bit for bit the image of the integer weights times 2^-22, and non-zero where they are
        layer = E.tap_layer(m)
        with L.operand("f16"):
            img = (layer.packed_eval(layer.fwd_form, bn)[0] if folded_form else layer.packed(layer.fwd_form)).cpu()
            ints_img = E.tap_layer(_module(r, c["w"])).packed(layer.fwd_form).cpu()
        assert img.dtype == F16 and torch.equal(img.double(), ints_img.double() * R.SUB_GAMMA)
        assert int((img != 0).sum()) == int((c["w"] != 0).sum()) and bool(sub(img.double()).sum() == (img != 0).sum())
    _assert_bits(got, exact, f"{name} gen{gen} subnormal {which}")


# ------------------------------------------------------------------------------------------------------------------ 3. overflow
@pytest.mark.parametrize("form", ["fold", "neg", "res"])
@pytest.mark.parametrize("key", [("1x1p", 5), ("3x3", 5), ("3x3", 6)], ids=_id)
def test_overflow(key, form):
    name, gen = key
    c = R.overflow_case(name, _ints)
    r, exact, gamma = c["route"], c["exact"][form], c["gamma"][form]
    R.assert_exact_in_fp32(r, c["x"], c["w"] * r.per_out_channel(gamma), None, 1.0, 1.0)
    s, S = R.shares(exact), c["sums"]
    top = 65504.0 / R.OVERFLOW_GAMMA[name]  # the sum whose product is the largest finite fp16 value; top + 1 becomes +inf
    assert int((S == top).sum()) >= 100 and int((S == top + 1).sum()) >= 100
    if name == "1x1p":
        assert 16.0 * (top + 1) == 65520.0  # the tie between 65504 and 2^16: rounds to the even neighbour, which is +inf
    if form == "fold":
        assert s["inf"] >= 0.2 and 1 - s["inf"] >= 0.2, s
    elif form == "neg":
        neg = gamma < 0
        assert bool((c["sums"][:, neg] * R.OVERFLOW_GAMMA[name] > 65520).float().mean() >= 0.2) and bool((exact[:, neg] == 0).all()) and s["inf"] >= 0.15
    else:
        y = c["exact"]["fold"].to(F16)
        assert bool(((y.isinf()) & (c["res"] == -32768.0)).float().mean() >= 0.04) and bool(exact[y.isinf()].isinf().all()) and bool(c["res"].isfinite().all())
    bn = _bn(r.cout, gamma)
    got = _launch(r, gen, ROUTE_GENS[key][1], c["x"], _module(r, c["w"]), bn, relu=True, res=c["res"] if form == "res" else None,
                  res_relus=(True, False) if form == "res" else None)
    assert not bool((got == -float("inf")).any())
    _assert_bits(got, exact, f"{name} gen{gen} overflow {form}")


# ------------------------------------------------------------------------------------------------------------------ 4. BatchNorm decades
def _launch_unfolded(r, gen, expect, x, module, bn, tag):
    """conv_bn on a layer the engine must NOT fold (TapLayer.eval_fold_ok): the plain conv, BatchNorm as a folded operand (a Lazy), which
    is written out here by the pass a consumer that cannot fold it uses.  The residual entry point declines the layer as well."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    dt = F16 if tag == "f16" else torch.bfloat16
    with _small_grids_allowed(gen), L.operand(tag):
        t = E.Tape(False, DEV)
        layer = E.tap_layer(module)
        assert not layer.eval_fold_ok(bn)
        xa = E.Act.from_nchw(x.to(dt).to(DEV))
        assert E.conv_bn_residual(t, layer, xa, bn, E.Act.empty(r.N, r.H, r.w_out, r.cout, DEV), False, True) is None and not t.ops
        y = E.conv_bn(t, layer, xa, bn, relu=True)
        assert isinstance(y, E.Lazy) and [type(o) for o in t.ops] == [E.ConvOp, E.BnOp] and t.ops[0].eval_bn is None
        assert layer.images.held(E.image_slot(layer.fwd_form, "eval_fold")) is None  # no folded image was built
        info = _planned(E, L, layer, t.ops[0])
        assert info[0] == expect, (info, expect)
        out = y.materialized().nchw().cpu()
        torch.cuda.synchronize()
    return out


# whether the engine folds the layer: always in the bf16 build; in the fp16 build only while the image holds the folded weights as
# well as the plain ones (scales down to 2^-9 here: "var" reaches 2^-10, "gamma" 2^-12)
_FOLDED = lambda which, tag: tag == "bf16" or which == "mid"


@pytest.mark.parametrize("tag", ["f16", "bf16"])
@pytest.mark.parametrize("which", ["var", "gamma", "mid"])
@pytest.mark.parametrize("key", [("3x3", 5), ("3x3", 6), ("1x1", 5)], ids=_id)
def test_bn_scales_over_decades(key, which, tag):
    """Random data, eval-mode BatchNorm scales over many decades ("var": running_var = 4^k, k in -10..10; "gamma": gamma = +-2^k, k in
    -12..6; "mid": running_var = 4^k, k in -8..8).  Every element within the derived bound of the route's contract, and every channel no
    further from fp64 BatchNorm than twice what the reference's route (16-bit conv output, BatchNorm in high precision) is.  In the fp16
    build "var" and "gamma" are layers the engine must not fold -- their folded weights underflow fp16's normal range, which cost up to
    7.5 x the reference route's error when they were folded -- and the test asserts that the unfolded route is taken and meets the
    same two checks; "mid" stays folded in both builds."""
    name, gen = key
    dt = F16 if tag == "f16" else torch.bfloat16
    c = R.decade_case(R.ROUTES[name], which, dt)
    r = c["route"]
    m, bn = _module(r, c["w"]), _bn(r.cout, *c["bn"])
    folded = _FOLDED(which, tag)
    if folded:
        got = _launch(r, gen, ROUTE_GENS[key][1], c["x"], m, bn, relu=True, tag=tag)
    else:
        got = _launch_unfolded(r, gen, ROUTE_GENS[key][0], c["x"], m, bn, tag)
    R.assert_decades(c, got, dt, f"{name} gen{gen} {which} {tag}", folded=folded)


# ------------------------------------------------------------------------------------------------------------------ 5. rescaled twin
def _conv_bn_pairs(*roots):
    """(name, conv, bn) of every conv -> BatchNorm pair, in module order (each BatchNorm follows its conv in every container here)."""
    pairs, prev = [], None
    for root in roots:
        for name, m in root.named_modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                prev = (name, m)
            elif isinstance(m, torch.nn.BatchNorm2d):
                assert prev is not None and prev[1].bias is None, name
                out_dim = 1 if isinstance(prev[1], torch.nn.ConvTranspose2d) else 0
                assert prev[1].weight.shape[out_dim] == m.num_features
                pairs.append((*prev, m))
                prev = None
    return pairs


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "unfolded"])
@pytest.mark.parametrize("tag", ["f16", "bf16"])
def test_rescaled_twin(golden, tag, fold):
    """The tiny detector (eps = 0) and a twin in which every conv -> BatchNorm pair has its conv rows, running_mean and sqrt(running_var)
    multiplied by a_c = 2^j per output channel.  The twin is the same function, and in this arithmetic the same BITS: a power of two
    commutes with every rounding involved (the fp64 fold, its sqrt, the 16-bit weight image, fp32 accumulation, the 16-bit stores) as
    long as nothing leaves the normal range of its format -- so a channel with a scale far from 1 is computed exactly as well as one at 1.
    j is drawn from -8..8, narrowed where the FORMAT (not the code) makes the scaling inexact:

    * fp16, any path that reads the conv's OWN weights as a 16-bit image (EVAL_FOLD off; the small-K, positional-pair and fusion layers
      of the stem): j stays where every non-zero weight of the channel is a normal fp16 number before and after (0 for a channel that
      has a weight below 2^-14 already: fp16 holds that one coarsely, its scaled copy finely).  Applied to every pair of the fp16 runs.
    * fp16, any path that stores the conv's raw output in 16 bits before the BatchNorm (EVAL_FOLD off: all; EVAL_FOLD on: the stem's
      positional pair and modulation): j >= 0 -- scaled down by 2^-8, every raw output below 2^-6 becomes an fp16 subnormal and loses bits.
      (Scaled UP, an output below 2^-14 gains bits; with 1024 pixels of unit-size outputs none is that small.)
    * bf16: the full range (its normal range ends at 2^-126)."""
    from range_view_3d_detection_amd import engine as E
    from test_gpu_model import load_tiny

    g = golden("tiny_model")
    dt = F16 if tag == "f16" else torch.bfloat16
    (b0, h0), (b1, h1) = load_tiny(g), load_tiny(g)
    gen = torch.Generator().manual_seed(5)
    js = []
    for (name, conv, bn), (_, conv0, bn0) in zip(_conv_bn_pairs(b1, h1), _conv_bn_pairs(b0, h0)):
        bn.eps = bn0.eps = 0.0
        c = bn.num_features
        out_dim = 1 if isinstance(conv, torch.nn.ConvTranspose2d) else 0
        w = conv.weight.data.cpu()
        lo, hi = torch.full((c,), -8), torch.full((c,), 8)
        if tag == "f16":
            rows = w.abs().transpose(0, out_dim).reshape(c, -1).double()
            wmin, wmax = torch.where(rows == 0, torch.inf, rows).amin(1), rows.amax(1)
            lo = torch.maximum(lo, torch.ceil(-14 - torch.log2(wmin)).long())
            hi = torch.minimum(hi, torch.floor(15 - torch.log2(wmax)).long())  # (2^15 max|w| < 65504)
            if not fold or name.startswith("stem."):
                lo = lo.clamp_min(0)
            lo, hi = torch.where(wmin < R.F16_MIN_NORMAL, 0, lo).clamp_max(0), torch.where(wmin < R.F16_MIN_NORMAL, 0, hi).clamp_min(0)
        j = lo + (torch.rand(c, generator=gen) * (hi - lo + 1).double()).floor().long().clamp_max(hi - lo)
        a = torch.pow(2.0, j.double()).float()
        w1 = w * (a.view(1, -1, 1, 1) if out_dim else a.view(-1, 1, 1, 1))
        if tag == "f16":  # no scaled weight leaves fp16's normal range (nor was outside it where j != 0)
            moved = (w1 != w) & (w != 0)
            assert bool((w1[moved].abs() >= R.F16_MIN_NORMAL).all()) and bool((w[moved].abs() >= R.F16_MIN_NORMAL).all()) and float(w1.abs().max()) < R.F16_MAX
        assert torch.equal(w1.double(), w.double() * (a.double().view(1, -1, 1, 1) if out_dim else a.double().view(-1, 1, 1, 1)))  # exact in fp32
        mean1, var1 = bn.running_mean.data.cpu() * a, bn.running_var.data.cpu() * a * a
        assert torch.equal(var1.double(), bn.running_var.data.cpu().double() * a.double() ** 2) and bool((var1 > 2.0 ** -100).all())
        conv.weight.data, bn.running_mean.data, bn.running_var.data = w1.to(DEV), mean1.to(DEV), var1.to(DEV)
        js.append(j)
    js = torch.cat(js)
    share = lambda m: float(m.float().mean())
    print(f"rescaled twin {tag} fold={fold}: {js.numel()} channels, j < 0 on {share(js < 0):.2f}, j > 0 on {share(js > 0):.2f}, |j| >= 4 on {share(js.abs() >= 4):.2f}")
    assert share(js > 0) >= 0.3 and share(js.abs() >= 4) >= 0.2 and (share(js < 0) >= (0.3 if tag == "bf16" else 0.1) or not fold)
    data = {"features": g["features"].to(DEV), "cart": g["cart"].to(DEV), "mask": g["mask"].to(DEV)}

    def run(backbone, head):
        backbone.eval()
        head.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=F16, enabled=tag == "f16"):
            out, _ = head(backbone(data), data, return_loss=False)
        return out[1][0]["logits"].float().cpu(), out[1][0]["regressands"].float().cpu()

    old = E.EVAL_FOLD
    E.EVAL_FOLD = fold
    try:
        (l0, r0), (l1, r1) = run(b0, h0), run(b1, h1)
    finally:
        E.EVAL_FOLD = old
    assert bool(l0.isfinite().all()) and bool(r0.isfinite().all()) and float(l0.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(r0, r1), (int((l0 != l1).sum()), float((l0 - l1).abs().max()), int((r0 != r1).sum()), float((r0 - r1).abs().max()), dt)
