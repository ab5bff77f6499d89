"""The data rules of test_gpu_fp16_edges.py, checked without a GPU: every generator of ``fp16_ref.py`` runs, and every share the GPU tests
assert before launching holds on the fp64 reference; the derived bound of the BatchNorm-decades test holds, with no exclusions, for a
float32 CPU convolution of the emulated fold at a reduced size (and the bound of the unfolded route the fp16 build falls back to, for
that route in float32)."""

from __future__ import annotations

import pytest
import torch

import fp16_ref as R

F16 = torch.float16
SMALL = {"3x3": R.Route("conv", 3, 1, 128, 256, 1, 8, 40), "1x1": R.Route("conv", 1, 1, 128, 256, 1, 8, 40)}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    R.release_cases()


def test_number_format_helpers():
    v = torch.tensor([0.0, 2.0 ** -24, 2.0 ** -14, 1.0, 1.5, 2047.0, 2048.0, 2049.0, 4097.0, 65504.0, 65519.0, 65520.0], dtype=torch.float64)
    assert R.spacing16(v).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 1.0, 2.0, 2.0, 4.0, 32.0, 32.0, 32.0]
    assert R.spacing16(torch.tensor([1.0, 3.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -6]
    h = R.to16(v)
    assert h.tolist()[-3:] == [65504.0, 65504.0, float("inf")] and float(h[1]) == 2.0 ** -24  # gradual underflow; the tie at 65520 is +inf
    assert float(R.to16(torch.tensor([2049.0, 2051.0], dtype=torch.float64))[0]) == 2048.0 and float(R.to16(torch.tensor([2051.0], dtype=torch.float64))[0]) == 2052.0
    s = R.shares(torch.tensor([[2049.0, 4097.0, 4098.0, 3.0 * 2.0 ** -24, 65520.0, 1.0]], dtype=torch.float64))
    assert s["ties"] == pytest.approx(2 / 6) and s["nonties"] == pytest.approx(1 / 6) and s["subnormal"] == pytest.approx(1 / 6) and s["inf"] == pytest.approx(1 / 6)
    with pytest.raises(AssertionError):
        R.to16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))


@pytest.mark.parametrize("name", sorted(R.ROUTES))
def test_rounding_data(name):
    c = R.rounding_case(name)
    r = c["route"]
    assert float(c["x"].min()) == 0 and float(c["w"].min()) == 0 and float(c["w"][:, ~c["wide"]].max() if r.kind == "convT" else c["w"][~c["wide"]].max()) == 1
    R.assert_exact_in_fp32(r, c["x"], c["w"], None, 1.0, 1.0)
    R.assert_exact_in_fp32(r, c["x"], c["wf"], c["shift"], 1.0, 0.5)
    assert torch.equal(c["shift"], c["shift"].round()) and set(c["gamma"].tolist()) == {0.5, 1.0, 2.0}
    for form, exact in c["exact"].items():
        s = R.assert_rounding_shares(exact, c["wide"], f"{name} {form}")
        print(name, form, {k: round(v, 3) for k, v in s.items()})
    # the rounding is observable: truncation, and rounding twice (through a 12-bit intermediate), both change the stored tensor
    e = c["exact"]["plain"]
    want = R.to16(e).double()
    trunc = torch.where(want > e, want - R.spacing16(e), want)
    assert float((trunc != want).float().mean()) > 0.05
    # the two residual forms differ from adding the residual before the one rounding
    y = R.fold64(R.conv64(r, c["x"], c["w"]), c["gamma"], c["beta"], c["mean"], True)
    assert float((R.to16(y + c["res"].double()) != R.to16(c["exact"]["res_conv"])).float().mean()) > 0.02


@pytest.mark.parametrize("name", R.SUB_ROUTES)
def test_subnormal_data(name):
    sub = lambda t: (t != 0) & (t.abs() < R.F16_MIN_NORMAL)
    a = R.subnormal_case(name, "weights")
    R.assert_exact_in_fp32(a["route"], a["x"], a["wf"], None, a["ux"], a["uw"])
    assert torch.equal(a["wf"].to(F16).double(), a["wf"].double()) and float(sub(a["wf"]).float().mean()) > 0.8  # the image is exact, and subnormal
    assert torch.equal(R.to16(a["exact"]).double(), a["exact"]) and float(a["exact"].abs().max()) < 2048 * R.F16_MIN_NORMAL
    assert float((a["exact"] != 0).float().mean()) >= 0.99
    # flushing the image to zero would store zeros only
    b = R.subnormal_case(name, "acts")
    R.assert_exact_in_fp32(b["route"], b["x"], b["wf"], None, b["ux"], b["uw"])
    s = R.shares(b["exact"])
    assert torch.equal(R.to16(b["exact"]).double(), b["exact"]) and s["subnormal"] >= 0.95 and float(sub(b["x"]).float().mean()) > 0.8
    print(name, "subnormal outputs of (b)", round(s["subnormal"], 4), "largest |sum| of (a) in units of 2^-14", float(a["exact"].abs().max()) * 2 ** 14)


@pytest.mark.parametrize("name", ["1x1p", "3x3"])
def test_overflow_data(name):
    c = R.overflow_case(name)
    r, S = c["route"], c["sums"]
    top = 65504.0 / R.OVERFLOW_GAMMA[name]
    assert top == int(top) and int((S == top).sum()) >= 100 and int((S == top + 1).sum()) >= 100
    s = {f: R.shares(e) for f, e in c["exact"].items()}
    assert s["fold"]["inf"] >= 0.2 and 1 - s["fold"]["inf"] >= 0.2
    h = R.to16(c["exact"]["fold"])
    assert bool((h[S == top] == 65504.0).all()) and bool(h[S == top + 1].isinf().all())
    neg = c["gamma"]["neg"] < 0
    assert int(neg.sum()) == r.cout // 4 and bool((c["exact"]["neg"][:, neg] == 0).all()) and s["neg"]["inf"] >= 0.15
    assert not any(bool(e.isnan().any()) or bool((e == -float("inf")).any()) for e in c["exact"].values())
    assert bool(c["exact"]["res"][h.isinf()].isinf().all()) and float((h.isinf() & (c["res"] == -32768.0)).float().mean()) >= 0.04
    # adding the residual in fp32 BEFORE the rounding would keep some of these finite: the case tells the two apart
    early = R.to16(c["exact"]["fold"] + c["res"].double())
    assert float((early != R.to16(c["exact"]["res"])).float().mean()) > 0.02
    print(name, {f: round(v["inf"], 3) for f, v in s.items()}, int((S == top).sum()), int((S == top + 1).sum()))


@pytest.mark.parametrize("dtype", [F16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("which", ["var", "gamma", "mid"])
@pytest.mark.parametrize("name", ["3x3", "1x1"])
def test_decades_bound_holds_for_a_float32_convolution(name, which, dtype):
    """The derived bound |got - emu| <= spacing(emu) + (n + 1) 2^-24 conv(|x|, |wf|) for torch's float32 convolution of the emulated
    fold: every element, no exclusions; no channel vacuous; the scales really span the decades."""
    c = R.decade_case(SMALL[name], which, dtype)
    gamma, beta, mean, var = c["bn"]
    scale = gamma.double() / var.double().sqrt()
    assert float(scale.abs().max() / scale.abs().min()) >= 2.0 ** 16 and (which != "gamma" or bool((scale < 0).sum() >= 256 // 3 - 1))
    got = R.fold_route_fp32(c, dtype).double()
    emu, bound = c["emu"], c["bound"]
    assert bool(((got - emu).abs() <= bound).all()), float(((got - emu).abs() / bound).max())
    top = emu.amax(dim=(0, 2, 3))
    assert bool((top > 8 * R.spacing16(top, dtype)).all())
    got_u = R.unfolded_route_fp32(c, dtype).double()
    assert bool(((got_u - c["emu_u"]).abs() <= c["bound_u"]).all()), float(((got_u - c["emu_u"]).abs() / c["bound_u"]).max())
    assert float((c["bound_u"].amax(dim=(0, 2, 3)) / R.spacing16(c["emu_u"].amax(dim=(0, 2, 3)), dtype)).max()) < 6.0
    # and the bound is no blanket: at most a few spacings of the storage type at the channel's own largest output
    assert float((bound.amax(dim=(0, 2, 3)) / R.spacing16(top, dtype)).max()) < 3.0
