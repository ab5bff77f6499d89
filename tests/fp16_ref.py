"""CPU side of test_gpu_fp16_edges.py: the routes, the data rules and the fp64 references of the tests at fp16's own edges.

Everything here is plain torch on the CPU.  ``test_fp16_ref_cpu.py`` runs every generator and checks every share the GPU tests rely
on, so that the data rules cannot drift while no GPU is looking.

* ``ROUTES``: the shapes that reach each kernel form (the generation is asserted in the GPU test, from ``rv_tap_launch_info``).
* ``conv64``: the convolution of a route in fp64, 'same' padding as ``Conv2dSame`` / ``ConvTranspose2d(padding=(1, 1))``.
* items 1-3: integer (or integer x power of two) data whose products and partial sums are exact in fp32 whatever the summation order
  (``assert_exact_in_fp32``); the expected store is the fp64 result cast ONCE to fp16 by torch's CPU cast (round to nearest even,
  gradual underflow, infinity beyond 65519.99...).  torch casts fp64 -> fp16 through fp32: that is one rounding only because the exact
  value fits fp32, which ``to16`` asserts.
* item 4: the fold contract ``wf = round16(float32(w) * float32(scale)); y = relu(conv_fp64(x, wf) + shift)`` rounded once, the per-element
  bound derived from fp32 accumulation, and the reference's own unfolded route (16-bit conv output, BatchNorm in high precision).
"""

from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

F64 = torch.float64
U24 = float(1 << 24)
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
F16_MIN_SUBNORMAL = 2.0 ** -24


class Route(NamedTuple):
    kind: str  # "conv" (Conv2dSame) | "convT" (ConvTranspose2d (3, 4), stride (1, 2), padding (1, 1))
    k: int  # square kernel size of a conv
    stride_w: int
    cin: int
    cout: int
    N: int
    H: int
    W: int

    @property
    def terms(self) -> int:
        """Products summed into one (interior) output."""
        return self.cin * (6 if self.kind == "convT" else self.k * self.k)  # convT: 3 rows x (4 columns / stride 2)

    @property
    def w_out(self) -> int:
        return self.W * 2 if self.kind == "convT" else self.W // self.stride_w

    def weight_shape(self) -> Tuple[int, ...]:
        return (self.cin, self.cout, 3, 4) if self.kind == "convT" else (self.cout, self.cin, self.k, self.k)

    def per_out_channel(self, v: torch.Tensor) -> torch.Tensor:
        """(cout,) -> broadcastable against the torch weight of this route."""
        return v.view(1, -1, 1, 1) if self.kind == "convT" else v.view(-1, 1, 1, 1)


# the smallest shapes at which each kernel still has full tiles, a border and a ragged edge (test_eval_fold_exact,
# test_residual_epilogue_equals_the_separate_pass); "g": the register-staged generic kernels
ROUTES: Dict[str, Route] = {
    "3x3": Route("conv", 3, 1, 128, 256, 2, 16, 256),
    "1x1": Route("conv", 1, 1, 128, 256, 2, 16, 256),
    "1x1p": Route("conv", 1, 1, 256, 256, 2, 32, 512),
    "3x3s2": Route("conv", 3, 2, 128, 256, 2, 16, 256),
    "convT": Route("convT", 3, 2, 128, 256, 2, 16, 256),
    "3x3g": Route("conv", 3, 1, 128, 256, 2, 4, 32),
    "1x1g": Route("conv", 1, 1, 128, 256, 2, 4, 32),
}


def ints(shape, g, lo, hi):
    """Integers in [lo, hi) as fp32 (the rule of ``_ints`` in test_gpu_tapconv4.py, which the GPU tests pass in)."""
    return torch.randint(lo, hi, shape, generator=g).float()


def conv64(r: Route, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The route's convolution in fp64."""
    x, w = x.to(F64), w.to(F64)
    if r.kind == "convT":
        return F.conv_transpose2d(x, w, stride=(1, 2), padding=(1, 1))
    if r.k == 1 and r.stride_w == 1:
        return torch.einsum("oc,nchw->nohw", w[:, :, 0, 0], x)
    t = r.k - 1
    return F.conv2d(F.pad(x, [t // 2, t - t // 2, t // 2, t - t // 2]), w, stride=(1, r.stride_w))


def ch(r: Route, v: torch.Tensor) -> torch.Tensor:
    return v.to(F64).view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ number formats
def spacing16(v: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """Distance from |v| to the next larger value of the 16-bit type (fp64; subnormal spacing at the bottom of fp16)."""
    bits, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    _, e = torch.frexp(v.to(F64).abs().clamp_min(2.0 ** -300))  # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v, dtype=F64), (e - 1).clamp_min(emin) - bits)


def to16(exact: torch.Tensor, dtype=torch.float16) -> torch.Tensor:
    """The exact fp64 value rounded ONCE to the storage type (the value has to fit fp32, through which torch's cast goes)."""
    assert torch.equal(exact.float().double(), exact), "the exact result does not fit fp32 (data rule)"
    return exact.to(dtype)


def assert_exact_in_fp32(r: Route, x: torch.Tensor, wf: torch.Tensor, shift: Optional[torch.Tensor], ux: float, uw: float) -> None:
    """x holds multiples of ``ux`` and the (folded) weights multiples of ``uw``, so every product and the shift are multiples of
    ux * uw; every partial sum, in any order, stays below 2^24 of these units: fp32 accumulation is exact."""
    whole = lambda t, u: torch.equal((t.to(F64) / u).round(), t.to(F64) / u)
    unit = ux * uw
    assert whole(x, ux) and whole(wf, uw) and (shift is None or whole(shift, unit)), "the data are not multiples of their units"
    total = conv64(r, x.abs(), wf.abs())
    if shift is not None:
        total = total + ch(r, shift).abs()
    assert float(total.max()) / unit < U24, (float(total.max()) / unit, U24)
    assert unit >= 2.0 ** -126  # (fp32's normal range: nothing here is an fp32 subnormal)


def shares(exact: torch.Tensor) -> Dict[str, float]:
    """Of the exact values: fractions above / below 2048 in magnitude, exact ties of the fp16 grid, values fp16 cannot hold that are no
    ties, non-zero subnormal results, overflows."""
    v = exact.to(F64)
    h = v.to(torch.float16).double()
    off = (v - h).abs()
    inexact = (off != 0) & h.isfinite()
    tie = inexact & (2 * off == spacing16(v))
    n = v.numel()
    return {"above": float((v.abs() > 2048).sum()) / n, "below": float((v.abs() < 2048).sum()) / n, "ties": float(tie.sum()) / n,
            "nonties": float((inexact & ~tie).sum()) / n, "subnormal": float(((h != 0) & (h.abs() < F16_MIN_NORMAL)).sum()) / n,
            "inf": float(h.isinf().sum()) / n}


# ------------------------------------------------------------------------------------------------------------------ item 1: rounding
# activations in [0, ACT_HI[route]): the sums of the {0, 1} channels sit around 2048 (from below), those of the {0, 1, 2} channels around
# 4096: terms x (hi - 1) / 2 x 1/2 ~ 2000 on every route.  (6 taps per conv-transpose output: 0..10 on the even input channels and 0..11
# on the odd ones, mean 5.25 -- 0..10 everywhere leaves the {0, 1, 2} channels below 4096, 0..11 everywhere the {0, 1} ones above 2048.)
ACT_HI = {"3x3": 8, "1x1": 64, "1x1p": 32, "3x3s2": 8, "convT": 11, "3x3g": 8, "1x1g": 64}


def wide_channels(r: Route) -> torch.Tensor:
    """The output channels whose weights are drawn from {0, 1, 2}: every other pair, so that each 16-channel MFMA tile has both kinds."""
    return (torch.arange(r.cout) // 2) % 2 == 1


def rounding_data(name: str, g, ints: Callable = ints):
    """(x, w): non-negative integers; half of the output channels take weights in {0, 1, 2}."""
    r = ROUTES[name]
    x = ints((r.N, r.cin, r.H, r.W), g, 0, ACT_HI[name])
    if name == "convT":
        x = torch.where((torch.arange(r.cin) % 2 == 1).view(1, -1, 1, 1), ints(x.shape, g, 0, ACT_HI[name] + 1), x)
    w = torch.where(r.per_out_channel(wide_channels(r)), ints(r.weight_shape(), g, 0, 3), ints(r.weight_shape(), g, 0, 2))
    return x, w


def exact_bn(c: int, g, ints: Callable = ints, gammas=(0.5, 1.0, 2.0)):
    """(gamma, beta, running_mean): with eps = 0 and running_var = 1 the fold is exact: scale = gamma in {0.5, 1, 2}, shift = beta -
    mean * gamma an integer (mean is even)."""
    gamma = torch.tensor(gammas)[torch.randint(0, len(gammas), (c,), generator=g)]
    return gamma, ints((c,), g, -4, 5), 2 * ints((c,), g, -1, 2)


def fold64(conv: torch.Tensor, gamma, beta, mean, relu: bool) -> torch.Tensor:
    """bn(conv) with eps = 0, var = 1 in fp64, ReLU on request."""
    y = conv * gamma.to(F64).view(1, -1, 1, 1) + (beta.to(F64) - mean.to(F64) * gamma.to(F64)).view(1, -1, 1, 1)
    return y.clamp_min(0) if relu else y


def residual64(y: torch.Tensor, res: torch.Tensor, relu_out: bool, dtype=torch.float16) -> torch.Tensor:
    """rv_tap_residual's contract: the conv result is rounded to the storage type, THEN the residual is added (and rounded by the store)."""
    s = to16(y, dtype).double() + res.to(F64)
    return s.clamp_min(0) if relu_out else s


ROUNDING_MIN = {"above": 0.20, "below": 0.20, "ties": 0.05}
ROUNDING_MIN_NONTIES_WIDE = 0.05


def assert_rounding_shares(exact: torch.Tensor, wide: torch.Tensor, what: str) -> Dict[str, float]:
    s = shares(exact)
    sw = shares(exact[:, wide])
    for k, lo in ROUNDING_MIN.items():
        assert s[k] >= lo, (what, k, s)
    assert sw["nonties"] >= ROUNDING_MIN_NONTIES_WIDE, (what, "non-ties in the {0, 1, 2} channels", sw)
    assert s["inf"] == 0 and float(exact.abs().max()) < F16_MAX
    return {**s, "nonties_wide": sw["nonties"]}


# ------------------------------------------------------------------------------------------------------------------ item 2: subnormals
SUB_GAMMA = 2.0 ** -22
SUB_ROUTES = ("3x3", "1x1", "1x1p", "3x3g", "1x1g")


def subnormal_weight_data(name: str, g, ints: Callable = ints):
    """(a): integer weights in -3..3 under a fold of 2^-22 (image: multiples of 2^-22 up to 3 x 2^-22, all fp16 subnormals), activations
    integers in -7..7 times 2^8.  Products are multiples of 2^-14."""
    r = ROUTES[name]
    return ints((r.N, r.cin, r.H, r.W), g, -7, 8) * 256.0, ints(r.weight_shape(), g, -3, 4)


def subnormal_act_data(name: str, g, ints: Callable = ints):
    """(b): activations integers in -3..3 times 2^-24 (fp16 subnormals), weights in {-1, 0, 1}: the sums are multiples of 2^-24, almost
    all of them below 2^-14 in magnitude."""
    r = ROUTES[name]
    return ints((r.N, r.cin, r.H, r.W), g, -3, 4) * F16_MIN_SUBNORMAL, ints(r.weight_shape(), g, -1, 2)


# ------------------------------------------------------------------------------------------------------------------ item 3: overflow
def overflow_data(name: str, g, ints: Callable = ints):
    """Non-negative integers, weights in {0, 1}: sums S around 4032 ("1x1p", activations 0..63, fold 16: 16 S around 64512) or around
    2016 ("3x3", activations 0..7, fold 32)."""
    r = ROUTES[name]
    return ints((r.N, r.cin, r.H, r.W), g, 0, {"1x1p": 64, "3x3": 8}[name]), ints(r.weight_shape(), g, 0, 2)


OVERFLOW_GAMMA = {"1x1p": 16.0, "3x3": 32.0}


# ------------------------------------------------------------------------------------------------------------------ item 4: BN decades
def decade_bn(c: int, which: str, g):
    """(gamma, beta, running_mean, running_var), eps = 0.  "var": running_var = 4^k, k cycling over -10..10, gamma = 1 (scale 2^-k);
    "gamma": running_var = 1, gamma = 2^k, k cycling over -12..6, negative on every third channel; "mid": as "var" with k in -8..8.  beta follows |scale| (0.1 |scale| randn, the
    conv's own deviation being 0.34 |scale| or more) so that a good part of every channel survives the ReLU at every scale."""
    i = torch.arange(c)
    if which == "var":
        var, gamma = torch.pow(4.0, (i % 21 - 10).double()).float(), torch.ones(c)
    elif which == "mid":  # the decades an fp16 image still holds with full precision (TapLayer.eval_fold_ok): scale 2^-8 .. 2^8
        var, gamma = torch.pow(4.0, (i % 17 - 8).double()).float(), torch.ones(c)
    else:
        var, gamma = torch.ones(c), torch.pow(2.0, (i % 19 - 12).double()).float() * torch.where(i % 3 == 2, -1.0, 1.0)
    scale = gamma.double() / var.double().sqrt()
    mean = 0.1 * torch.randn(c, generator=g)
    beta = (0.1 * torch.randn(c, generator=g).double() * scale.abs()).float()
    return gamma, beta, mean, var


def decade_data(r: Route, g, dtype):
    """x = randn rounded to the operand type, w = 0.03 randn (fp32 parameters)."""
    return torch.randn(r.N, r.cin, r.H, r.W, generator=g).to(dtype).float(), 0.03 * torch.randn(r.weight_shape(), generator=g)


def fold_scale_shift(gamma, beta, mean, var, eps: float = 0.0):
    """The engine's fold (TapLayer.packed_eval): scale and shift formed in fp64, handed to the packer / the epilogue as fp32."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale.float(), (beta.double() - mean.double() * scale).float()


def fold_emulation(r: Route, x, w, gamma, beta, mean, var, dtype, relu: bool = True):
    """The contract of the folded route.  Returns (emu: the exact value of the contract rounded once to ``dtype``, as fp64;
    bound: per-element |got - emu| allowed; wf)."""
    scale, shift = fold_scale_shift(gamma, beta, mean, var)
    wf = (w.float() * r.per_out_channel(scale)).to(dtype).float()
    y = conv64(r, x, wf) + ch(r, shift)
    mag = conv64(r, x.abs(), wf.abs()) + ch(r, shift).abs()
    if relu:
        y = y.clamp_min(0)
    emu = y.float().to(dtype).double()  # (fp64 -> fp32 -> 16 bits: torch's cast; the first step moves the value by 2^-24 relative at most)
    # fp32 accumulation of n products (exact each) and the shift, in any order: |error| <= (n + 1) 2^-24 sum |terms|; then ONE rounding
    # to the storage type on each side, which moves two values this close apart by one spacing at the most
    bound = spacing16(emu, dtype) + (r.terms + 1) * 2.0 ** -24 * mag
    return emu, bound, wf


def bn64(r: Route, x, w, gamma, beta, mean, var, relu: bool = True):
    """conv -> BatchNorm(eval, eps = 0) -> ReLU in fp64 from the fp32 parameters: what both routes approximate."""
    y = (conv64(r, x, w) - ch(r, mean)) / ch(r, var).sqrt() * ch(r, gamma) + ch(r, beta)
    return y.clamp_min(0) if relu else y


def unfolded_route(r: Route, x, w, gamma, beta, mean, var, dtype, relu: bool = True):
    """The reference's route under autocast: the conv with 16-bit weights and a 16-bit output (fp32 accumulation: emulated by the exact
    sum rounded once), BatchNorm on that tensor in high precision, ReLU, a 16-bit store."""
    c16 = conv64(r, x, w.to(dtype)).float().to(dtype).double()
    y = (c16 - ch(r, mean)) / ch(r, var).sqrt() * ch(r, gamma) + ch(r, beta)
    if relu:
        y = y.clamp_min(0)
    return y.float().to(dtype).double()


def unfolded_emulation(r: Route, x, w, gamma, beta, mean, var, dtype, relu: bool = True):
    """The contract of the engine's unfolded eval route: the conv with the plain 16-bit image and a 16-bit output, then
    relu(scale * c + shift) in fp32 with the fp32 scale and shift of ``fold_scale_shift``, stored in 16 bits.  Returns (emu, bound)."""
    scale, shift = fold_scale_shift(gamma, beta, mean, var)
    w16 = w.to(dtype).float()
    c16 = conv64(r, x, w16).float().to(dtype).double()
    mag = conv64(r, x.abs(), w16.abs())
    y = c16 * ch(r, scale) + ch(r, shift)
    if relu:
        y = y.clamp_min(0)
    emu = y.float().to(dtype).double()
    # the kernel's 16-bit conv output is within one spacing (+ the fp32 accumulation error) of c16; the affine pass multiplies that by
    # |scale| and adds two fp32 roundings (product and sum, or one FMA); then one rounding to the storage type on each side
    dc = spacing16(c16, dtype) + r.terms * 2.0 ** -24 * mag
    bound = spacing16(emu, dtype) + ch(r, scale).abs() * dc + 2.0 ** -23 * (ch(r, scale).abs() * (c16.abs() + dc) + ch(r, shift).abs())
    return emu, bound


def channel_error(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Per channel: max |got - want| over the channel's own max |want|."""
    return (got.double() - want).abs().amax(dim=(0, 2, 3)) / want.abs().amax(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------------------------ cases, built once
_CASES: Dict[tuple, dict] = {}
RES_FORMS = {"res_out": (False, True), "res_conv": (True, False)}  # form -> (ReLU on the conv, ReLU after the sum)


def _seed(*key) -> int:
    return sum(ord(ch_) * (i + 1) for i, ch_ in enumerate("/".join(map(str, key)))) % 100003


def rounding_case(name: str, ints: Callable = ints) -> dict:
    """Item 1 on one route: the data and the exact fp64 value each form stores ("plain", "fold", "res_out", "res_conv"), shared by the
    tests of every form and generation."""
    key = ("rounding", name)
    if key not in _CASES:
        r = ROUTES[name]
        g = torch.Generator().manual_seed(_seed(*key))
        x, w = rounding_data(name, g, ints)
        gamma, beta, mean = exact_bn(r.cout, g, ints)
        res = ints((r.N, r.cout, r.H, r.w_out), g, 0, 64)
        conv = conv64(r, x, w)
        exact = {"plain": conv, "fold": fold64(conv, gamma, beta, mean, True)}
        for form, (relu_conv, relu_out) in RES_FORMS.items():
            exact[form] = residual64(fold64(conv, gamma, beta, mean, relu_conv), res, relu_out)
        _CASES[key] = {"route": r, "x": x, "w": w, "gamma": gamma, "beta": beta, "mean": mean, "res": res, "exact": exact,
                       "wide": wide_channels(r), "wf": w * r.per_out_channel(gamma), "shift": beta - mean * gamma}
    return _CASES[key]


def subnormal_case(name: str, which: str, ints: Callable = ints) -> dict:
    """Item 2 on one route.  "weights" (a): fold 2^-22 on integer weights, no ReLU, zero shift -- "wf" is the folded fp32 weight, whose
    fp16 image is exact; "acts" (b): plain store of sums of subnormal activations.  "exact": what is stored, representable in fp16."""
    key = ("subnormal", name, which)
    if key not in _CASES:
        r = ROUTES[name]
        g = torch.Generator().manual_seed(_seed(*key))
        if which == "weights":
            x, w = subnormal_weight_data(name, g, ints)
            wf, ux, uw = w * SUB_GAMMA, 256.0, SUB_GAMMA
        else:
            x, w = subnormal_act_data(name, g, ints)
            wf, ux, uw = w, F16_MIN_SUBNORMAL, 1.0
        _CASES[key] = {"route": r, "x": x, "w": w, "wf": wf, "ux": ux, "uw": uw, "exact": conv64(r, x, wf)}
    return _CASES[key]


def overflow_case(name: str, ints: Callable = ints) -> dict:
    """Item 3 on "1x1p" (fold 16) or "3x3" (fold 32).  Forms: "fold" (ReLU), "neg" (the fold negated on every fourth channel, ReLU:
    -inf must store 0), "res" (ReLU on the conv, then a finite residual -- integers in -2048..2047, -32768 on every fifth pixel column:
    inf + finite stays inf because the conv result is rounded to fp16 BEFORE the sum)."""
    key = ("overflow", name)
    if key not in _CASES:
        r = ROUTES[name]
        g = torch.Generator().manual_seed(_seed(*key))
        x, w = overflow_data(name, g, ints)
        gamma = torch.full((r.cout,), OVERFLOW_GAMMA[name])
        gamma_neg = torch.where(torch.arange(r.cout) % 4 == 3, -gamma, gamma)
        zero = torch.zeros(r.cout)
        res = ints((r.N, r.cout, r.H, r.w_out), g, -2048, 2048)
        res[..., ::5] = -32768.0
        conv = conv64(r, x, w)
        y = fold64(conv, gamma, zero, zero, True)
        exact = {"fold": y, "neg": fold64(conv, gamma_neg, zero, zero, True),
                 "res": y.to(torch.float16).double() + res.double()}  # (y fits fp32: integers below 2^24)
        _CASES[key] = {"route": r, "x": x, "w": w, "gamma": {"fold": gamma, "neg": gamma_neg, "res": gamma}, "res": res, "sums": conv, "exact": exact}
    return _CASES[key]


def decade_case(r: Route, which: str, dtype) -> dict:
    """Item 4: the data, the contract's value and bound, the fp64 BatchNorm and the per-channel error of the reference's unfolded route."""
    key = ("decades", r, which, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(_seed("decades", r.k, r.cin, which))
        x, w = decade_data(r, g, dtype)
        bn = decade_bn(r.cout, which, g)
        emu, bound, wf = fold_emulation(r, x, w, *bn, dtype)
        emu_u, bound_u = unfolded_emulation(r, x, w, *bn, dtype)
        y64 = bn64(r, x, w, *bn)
        _CASES[key] = {"route": r, "x": x, "w": w, "bn": bn, "emu": emu, "bound": bound, "wf": wf, "y64": y64, "emu_u": emu_u, "bound_u": bound_u,
                       "ref_route_error": channel_error(unfolded_route(r, x, w, *bn, dtype), y64)}
    return _CASES[key]


def fold_route_fp32(c: dict, dtype) -> torch.Tensor:
    """The folded route in fp32 on the CPU (torch's convolution: some summation order, FMA or not): a stand-in for the kernel."""
    r = c["route"]
    scale, shift = fold_scale_shift(*c["bn"])
    x, wf = c["x"].float(), c["wf"].float()
    if r.kind == "convT":
        y = F.conv_transpose2d(x, wf, stride=(1, 2), padding=(1, 1))
    else:
        t = r.k - 1
        y = F.conv2d(F.pad(x, [t // 2, t - t // 2, t // 2, t - t // 2]), wf, stride=(1, r.stride_w))
    return (y + shift.view(1, -1, 1, 1)).clamp_min(0).to(dtype)


def unfolded_route_fp32(c: dict, dtype) -> torch.Tensor:
    """The engine's unfolded eval route in fp32 on the CPU: conv -> 16 bits -> fp32 affine + ReLU -> 16 bits."""
    r = c["route"]
    scale, shift = fold_scale_shift(*c["bn"])
    x, w16 = c["x"].float(), c["w"].to(dtype).float()
    t = r.k - 1
    c16 = F.conv2d(F.pad(x, [t // 2, t - t // 2, t // 2, t - t // 2]), w16, stride=(1, r.stride_w)).to(dtype).float()
    return (c16 * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).clamp_min(0).to(dtype)


def assert_decades(c: dict, got: torch.Tensor, dtype, what: str, folded: bool = True) -> str:
    """The checks of item 4 on a result of the folded route (``folded=False``: of the unfolded route the engine falls back to);
    returns the line of figures."""
    got = got.double()
    emu, bound, y64 = (c["emu"], c["bound"], c["y64"]) if folded else (c["emu_u"], c["bound_u"], c["y64"])
    # no channel is vacuous: its largest output is more than 8 spacings of the storage type at that value
    top = emu.amax(dim=(0, 2, 3))
    assert bool((top > 8 * spacing16(top, dtype)).all()), (what, "a channel without a significant output")
    assert bool(got.isfinite().all()) and bool(emu.isfinite().all()), what
    over = (got - emu).abs() - bound
    assert float(over.max()) <= 0, (what, "beyond the derived bound", int((over > 0).sum()), float(((got - emu).abs() / bound).max()))
    e_fold, e_ref = channel_error(got, y64), c["ref_route_error"]
    worst = int((e_fold / e_ref).argmax())
    line = (f"{what}: {'fold' if folded else 'unfolded (fallback)'} route vs fp64 BatchNorm, per channel of its own maximum: median {float(e_fold.median()):.2e} max {float(e_fold.max()):.2e}; "
            f"reference's unfolded route: median {float(e_ref.median()):.2e} max {float(e_ref.max()):.2e}; worst ratio {float((e_fold / e_ref).max()):.2f} "
            f"(channel {worst}); subnormal share of the weight image {float(((c['wf'] != 0) & (c['wf'].abs() < F16_MIN_NORMAL)).float().mean()) if dtype == torch.float16 else 0.0:.3f}")
    print(line)
    assert bool((e_fold <= 2 * e_ref).all()), (what, "a channel further from fp64 BatchNorm than twice the reference's route", line)
    return line


def release_cases() -> None:
    _CASES.clear()
