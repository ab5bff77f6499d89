"""The loss KINDS of the fused detection loss (``csrc/loss.hip``: ``rv_detection_loss_table_forward`` / ``_backward`` with ``rvLossKinds``)
against the fp64 reference of ``loss_kinds_ref.py``, through the C ABI, with the harness of ``test_gpu_loss_kernels.py`` (NaN-filled
outputs with guard rows, NaN in the padding columns of the inputs).

EXACT, whatever the kinds: the foreground map; sums [3], [12], [13], [14] = 0, [15] = 1 per row and in the totals row, whose [0..11] are 0;
with affinity maps the soft targets, bit for bit the map value at the label; both gradients exactly 0 where ``mask == 0``;
``d_regressands`` exactly 0 where the label is background or ``r == t``; the padding columns as ``include/rv3d.h`` states; guard rows.
L1: ``d_regressands`` within one fp32 ulp of ``float(reference)`` plus one per backward factor, sums [4..11] / [20..23] to relative 1e-12.
Kinds {0, 0} through the new pair: every tensor bit for bit what the multilevel pair (and the ``_aff`` pair) returns, rows to 1e-12.

MEASURED against the reference, in the units of ``loss_kinds_ref`` (fp32 ulps of the sum of the absolute addends): the regression
gradients and sums of SMOOTH_L1 / HUBER / MSE, sums [0..2], the scalars [16..23], ``d_logits`` per stratum.  Bound: twice the worst figure
of the SAME definition in fp32 torch on the CPU (``loss_kinds_ref.torch32_loss``) over ``loss_kinds_ref.yardstick_cases`` and on the case's
own inputs, no less than 4 ulp, one more per fp32 multiplication of the backward factors.  fp32 torch forms 1 - p by subtraction and its
BCE cancels, so it is no yardstick where p rounds to 1 or x is far negative; there the bounds come from the precision of the formats
(``loss_kinds_ref.KIND_ULP`` = 64, ``loss_ref.TAIL_ULP`` = 40): ``d_logits`` of FOCAL / PENALTY_REDUCED is held to ``KIND_ULP`` where
``t == 0`` and to ``KIND_ULP`` plus the soft targets' bound where ``t > 0`` (there ``t`` is an input the kernel computes itself), the tail
stratum of every kind to ``TAIL_ULP``.  Worst figures (fp32 torch: an x86-64 host, over the yardstick cases; kernel: an MI355X, over
every case of this module -- ``pytest -s`` prints them):

    quantity                        fp32 torch (CPU)              bound (floor)         kernel (MI355X)
                                    vfl     focal   pen.red.      vfl   focal  p.r.     vfl    focal  p.r.
    sums [0..2] / scalars [16..19]  1.01    1.55    2.37          4     4      4.73     0.40   1.35   0.52
    d_logits, t > 0                 2.67    5.63    4.79e3        5.34  11.3   91.7     2.67   5.30   4.95
    d_logits, t == 0, x >= -2       17.9    22.4    24.6          35.8  44.8   49.2     18.0   8.23   7.92
    d_logits, t == 0, x < -2        1.28e6  8.54e6  9.21e6        40    40     40       7.40   9.53   8.81
                                    smooth  huber   mse           smooth huber mse      smooth huber  mse
    sums [4..11] / scalars [20..23] 0.061   0.193   0.259         4     4      4        0.13   0.50   0.43
    d_regressands                   1.57    1.70    1.71          4     4      4        1.47   1.38   1.97
    d_regressands, L1               (not measured)                1 (+1 per factor)     0
    soft targets (Gaussian)         (loss_ref's yardstick: 13.8)  27.7                  1.33

The largest bounds applied over the module (a case's own inputs and the backward factors raise the floor): sums / scalars 4.73,
``d_logits`` 93.7 (PENALTY_REDUCED, ``t > 0``, two factors) / 57.7 / 42, ``d_regressands`` 6.

Shapes: ``make_entry`` at 2x5x67 (three workgroups, the last one ragged) and a hand-made 1x1x5; row forms (26 classes, ld 32, ld_reg 8),
(3, 32, 32), (7, 40, 12).  Every case plants, and asserts that it holds at least one of each: an instance pixel whose regressands equal
its targets (affinity exactly 1 under azimuth-invariant targets; in the map form a map value of exactly 1), residuals with ``|d|`` exactly
``beta`` / ``delta`` (= 0.125), residuals below half of it and residuals above twice it.

Mutations of the new code, one value-only change each, run once on an MI355X; what caught each:

* ``(1-t)^4`` -> ``(1-t)^2``: 26 failed, every PENALTY_REDUCED case ....... test_cross_of_kinds[penalty_reduced-l1], sums [0..2] off by 3.9e4 ulp
* ``t == 1`` -> ``t > 0`` (PENALTY_REDUCED): 26 failed ..................... test_cross_of_kinds[penalty_reduced-l1], sums [0..2] off by 1.1e6 ulp
* SMOOTH_L1 ``|d| < beta`` -> ``<=`` with ``|d| - beta / 4`` outside: 33 failed, every SMOOTH_L1 case with beta > 0
  .......................................................................... test_cross_of_kinds[varifocal-smooth_l1], loss [16] off by 267 ulp
* ``alpha_t`` dropped (FOCAL): 20 failed, every FOCAL case with alpha >= 0 .. test_cross_of_kinds[focal-l1], sums [0..2] off by 4.8e6 ulp
* kinds ignored in backward only: 62 failed, all but the refusals and the cases at kinds {0, 0}
  .......................................................................... test_cross_of_kinds[varifocal-smooth_l1], d_regressands off by 1.8e9 ulp
* HUBER's gradient outside ``delta`` -> ``sign(d)``: 14 failed, every HUBER case
  .......................................................................... test_cross_of_kinds[varifocal-huber], d_regressands off by 1.1e8 ulp
"""

from __future__ import annotations

import ctypes
import math

import pytest
import torch

import loss_kinds_ref as K
import loss_ref as R
import test_gpu_loss_kernels as T
from test_gpu_forward import DEV

pytestmark = pytest.mark.gpu
WORST = {}
APPLIED = {}
C = K.THRESHOLD
CODING = R.DEFAULT.replace(coding_weights=R.CODING)
CLS_PARAMS = {K.CLS_VARIFOCAL: CODING, K.CLS_FOCAL: CODING.replace(alpha=0.25), K.CLS_PENALTY_REDUCED: CODING.replace(alpha=1.0)}


def _L():
    from range_view_3d_detection_amd import _lib as L

    return L


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nloss kinds vs loss_kinds_ref, worst fp32 ulps: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items()))
              + "; fp32 torch over the yardstick cases: " + "; ".join(f"{g}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(w.items()))
                                                                       for g, w in sorted(K.torch32_yardstick().items()))
              + "; largest bound applied: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(APPLIED.items())))


def _kinds(k: K.Kinds):
    return _L().LossKinds(k.cls_kind, k.reg_kind, k.reg_param)


def _run(devs, p, kinds: K.Kinds, grad_scale=1.0, device_factor=1.0):
    """``rv_detection_loss_table_forward`` / ``_backward`` (with maps when the entries carry them); (rows (n + 1, 24), the sums buffer)."""
    L, n = _L(), len(devs)
    sums = T._Buf((n + 1) * R.SUMS_LEN, torch.float64, guard=R.SUMS_LEN)
    table = (L.LossEntry * n)(*[d.struct() for d in devs])
    params, kk = T._params(p), _kinds(kinds)
    maps = (ctypes.c_void_p * n)(*[d.aff.data_ptr() for d in devs]) if devs[0].aff is not None else None
    L.call("rv_detection_loss_table_forward", table, n, ctypes.byref(params), ctypes.byref(kk), maps, L.ptr(sums.t), L.stream_ptr())
    torch.cuda.synchronize()
    rows = sums.body(n + 1, R.SUMS_LEN)
    if device_factor != 1.0:
        sums.t[n * R.SUMS_LEN + 15] = device_factor
    L.call("rv_detection_loss_table_backward", table, n, ctypes.byref(params), ctypes.byref(kk), maps, L.ptr(sums.t), grad_scale, L.stream_ptr())
    torch.cuda.synchronize()
    return rows, sums


def _measured(fig, bounds, extra, what, kinds):
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(fig.items())))
    for k, v in fig.items():
        tag = f"{k}[{K.CLS_NAMES[kinds.cls_kind] if k in K.CLS_KEYS or k == 'loss' else K.REG_NAMES[kinds.reg_kind] if k in K.REG_KEYS else ''}]"
        WORST[tag] = max(WORST.get(tag, 0.0), v)
        more = extra if k.startswith("d_") else 0
        APPLIED[tag] = max(APPLIED.get(tag, 0.0), bounds[k] + more)
        assert v <= bounds[k] + more, f"{what}: {k} is off by {v:.4g} fp32 ulp (bound {bounds[k] + more:.4g})"


def _check(ref: K.TableResult, devs, rows, sums, p, kinds: K.Kinds, what, grad_scale=1.0, device_factor=1.0, planted=True):
    n = len(devs)
    own = [K.torch32_figures(d.e, p, kinds, None if d.aff is None else d.aff.cpu()) for d in devs]
    per_entry = [K.kernel_bounds(kinds, f) for f in own]
    bounds = K.kernel_bounds(kinds, {k: max(f.get(k, 0.0) for f in own) for k in K.CLS_KEYS + K.REG_KEYS + ("soft",)})
    extra = int(grad_scale != 1.0 or device_factor != 1.0) + int(grad_scale != 1.0 and device_factor != 1.0)
    l1 = kinds.reg_kind == K.REG_L1
    assert sums.guard_ok(), f"{what}: wrote behind the sums"
    for k in range(n + 1):
        got, want = rows[k], ref.rows[k]
        for j in (3, 12, 13, 14, 15):
            assert float(got[j]) == float(want[j]), f"{what}: row {k} [{j}] = {float(got[j])!r}, expected {float(want[j])!r}"
        idx = ((0, 1, 2) if k < n else ()) + (16, 17, 18, 19)
        if l1:
            T._rel12(got[20:24], want[20:24], f"{what}: row {k} [20..23]")
            if k < n:
                T._rel12(got[4:12], want[4:12], f"{what}: row {k} [4..11]")
        else:
            idx += (tuple(range(4, 12)) if k < n else ()) + (20, 21, 22, 23)
        if k == n:
            assert bool((got[:12] == 0).all()), f"{what}: totals row [0..11]"
        _measured(K.figures(ref, k, row={j: float(got[j]) for j in idx}), bounds, 0, f"{what} row {k}", kinds)
    seen = {"t_is_1": 0, "at_threshold": 0, "inside": 0, "outside": 0, "t_between": 0}
    for k, d in enumerate(devs):
        e, er, w = d.e, ref.entries[k], f"{what} entry {k}"
        B, H, W = e.shape
        n_cls, row32 = e.n_cls, e.ld_logits == 32
        for buf, name in zip(d.outputs(), ("soft targets", "foreground", "d_logits", "d_regressands")):
            assert buf.guard_ok(), f"{w}: wrote behind the {name}"
        assert torch.equal(d.fg.body(B, H, W).double(), er.foreground), f"{w}: foreground map"
        soft = d.soft.body(B, n_cls, H, W)
        d_l, d_r = d.d_l.body(B, H, W, e.ld_logits), d.d_r.body(B, H, W, e.ld_reg)
        if d.aff is not None:
            one_hot = e.labels[:, None] == torch.arange(n_cls).view(1, n_cls, 1, 1)
            amap = d.aff.cpu()
            assert torch.equal(soft, torch.where(one_hot, amap[:, None].expand_as(soft), torch.zeros(()))), f"{w}: soft targets are not the map value at the label"
            fig = K.figures(ref, k, d_logits=d_l[..., :n_cls])
        else:
            fig = K.figures(ref, k, soft=soft, d_logits=d_l[..., :n_cls])
        assert bool(d_r[..., 8:].isnan().all()), f"{w}: columns 8.. of d_regressands were written"
        if row32:
            assert bool((d_l[..., n_cls:] == 0).all()), f"{w}: padding columns of d_logits (32-float rows) are not all zero"
        else:
            assert bool(d_l[..., n_cls:].isnan().all()), f"{w}: padding columns of d_logits (scalar form) were written"
        off = e.mask == 0
        assert bool((d_l[..., :n_cls][off] == 0).all()) and bool((d_r[..., :8][off] == 0).all()), f"{w}: gradient where mask == 0"
        g_r, want_r = d_r[..., :8].double(), er.d_regressands
        r_is_t = e.regressands[..., :8] == e.reg_targets.permute(0, 2, 3, 1)
        zero = (e.labels == n_cls)[..., None] | r_is_t | off[..., None]
        assert bool((want_r[zero] == 0).all()) and bool((want_r[~zero] != 0).all())
        assert bool((g_r[zero] == 0).all()), f"{w}: d_regressands where the label is background or r == t"
        if l1:
            err = (g_r - want_r.float().double()).abs() / R.ulp32(want_r)
            worst = float(torch.nan_to_num(err, nan=math.inf).max())
            WORST["d_regressands[l1]"] = max(WORST.get("d_regressands[l1]", 0.0), worst)
            assert worst <= 1 + extra, f"{w}: d_regressands (L1) is off by {worst:.3g} fp32 ulp (allowed {1 + extra})"
        else:
            fig.update(K.figures(ref, k, d_regressands=g_r))
        _measured(fig, per_entry[k], extra, w, kinds)
        for key, v in K.planted_report(e, er, C).items():
            seen[key] += v
    if planted:
        print(f"{what}: planted {seen}")
        for key in ("t_is_1", "at_threshold", "inside", "outside") + (("t_between",) if kinds.cls_kind == K.CLS_PENALTY_REDUCED else ()):
            assert seen[key] >= 1, f"{what}: the case holds no {key}"


def _case(entries, p, kinds, what, maps=None, **kw):
    devs = [T._Dev(e, None if maps is None else maps[k]) for k, e in enumerate(entries)]
    rows, sums = _run(devs, p, kinds, **kw)
    ref = K.loss_table(entries, p, kinds, aff_maps=maps, **kw)
    _check(ref, devs, rows, sums, p, kinds, what, **kw)
    return ref, devs, rows


def tiny_entry(seed: int, n_cls: int, ld: int, ld_reg: int) -> R.Entry:
    """1x1x5 by hand on top of ``make_entry``'s points and logits: two instances (pixels 0-2 and 3-4); pixel 0: regressands == targets;
    pixel 1: every residual beyond the first three exactly +-C, the first three tiny (0 < t < 1); pixel 2: residuals C / 8; pixel 3:
    residuals 4 C beyond the first three; pixel 4: as pixel 3 with mask 0."""
    e = R.make_entry(seed, 1, 1, 5, n_cls, ld, ld_reg)
    e.panoptics[:] = torch.tensor([1, 1, 1, 2, 2]).view(1, 1, 5)
    e.labels[:] = torch.tensor([0, 0, 0, n_cls - 1, n_cls - 1]).view(1, 1, 5)
    e.points_per_obj[:] = torch.tensor([3, 3, 3, 2, 2]).view(1, 1, 5)
    e.num_objects = 2
    e.mask[:] = torch.tensor([1, 1, 1, 1, 0], dtype=torch.uint8).view(1, 1, 5)
    g = torch.Generator().manual_seed(seed)
    tg = torch.round((torch.rand((1, 8, 1, 5), generator=g) * 2 - 1) * 64) / 64
    e.reg_targets[:] = tg
    sign = (torch.randint(0, 2, (1, 1, 5, 8), generator=g) * 2 - 1).float()
    res = torch.zeros((1, 1, 5, 8))
    res[0, 0, 1, :3], res[0, 0, 1, 3:] = 2.0 ** -6, C
    res[0, 0, 2] = C / 8
    res[0, 0, 3, :3], res[0, 0, 3, 3:] = 2.0 ** -5, 4 * C
    res[0, 0, 4] = res[0, 0, 3]
    e.regressands[..., :8] = tg.permute(0, 2, 3, 1) + sign * res
    assert bool(((e.regressands[..., :8] - tg.permute(0, 2, 3, 1)).abs() == res).all())
    e.logits[0, 0, 0, 0], e.logits[0, 0, 1, 0] = 30.0, -2.5  # the own class of a t == 1 pixel far out, of a 0 < t < 1 pixel in the tail region
    e.planted["exact"] = torch.tensor([1, 0, 0, 0, 0], dtype=torch.bool).view(1, 1, 5)
    return e


# ================================================================================================================== one entry
@pytest.mark.parametrize("reg_kind", range(4), ids=K.REG_NAMES)
@pytest.mark.parametrize("cls_kind", range(3), ids=K.CLS_NAMES)
def test_cross_of_kinds(cls_kind, reg_kind):
    """The full 3 x 4 cross at 26 classes in 32-float rows, 2x5x67."""
    kinds = K.Kinds(cls_kind, reg_kind, C if reg_kind in (K.REG_SMOOTH_L1, K.REG_HUBER) else 0.0)
    e = K.make_kind_entry(3000 + 4 * cls_kind + reg_kind, 2, 5, 67, 26, 32, 8)
    _case([e], CLS_PARAMS[cls_kind], kinds, f"{kinds.name}, 26 classes ld 32")


@pytest.mark.parametrize("dims", [(2, 5, 67), (1, 1, 5)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("form", K.FORMS, ids=lambda f: f"{f[0]}cls-ld{f[1]}")
@pytest.mark.parametrize("cls_kind", range(3), ids=K.CLS_NAMES)
def test_row_forms(cls_kind, form, dims):
    """Every classification kind in both class loops (32-float rows unrolled, every other row length scalar), ld_reg 8 / 32 / 12, three
    workgroups with a ragged last one and one wave of five lanes; the regression kind cycles."""
    reg_kind = (1 + cls_kind + K.FORMS.index(form) + (dims[0] == 1)) % 4
    kinds = K.Kinds(cls_kind, reg_kind, C if reg_kind in (K.REG_SMOOTH_L1, K.REG_HUBER) else 0.0)
    e = tiny_entry(3100 + form[0], *form) if dims == (1, 1, 5) else K.make_kind_entry(3100 + 10 * cls_kind + form[0], *dims, *form)
    _case([e], CLS_PARAMS[cls_kind], kinds, f"{kinds.name}, {form}, {dims}")


@pytest.mark.parametrize("form", [(26, 32, 8), (7, 40, 12)], ids=lambda f: f"{f[0]}cls-ld{f[1]}")
@pytest.mark.parametrize("gamma", [1.0, 2.0, 3.0, 1.5])
@pytest.mark.parametrize("cls_kind,alpha", [(K.CLS_FOCAL, 0.25), (K.CLS_FOCAL, -1.0), (K.CLS_PENALTY_REDUCED, 0.5)], ids=["focal", "focal-no-alpha", "penalty_reduced"])
def test_gamma_alpha(cls_kind, alpha, gamma, form):
    """The product paths (gamma 1, 2, 3), ``powf`` (1.5) and FOCAL without the alpha_t factor."""
    kinds = K.Kinds(cls_kind, K.REG_SMOOTH_L1, C)
    e = K.make_kind_entry(3200 + form[0], 2, 5, 67, *form)
    _case([e], CODING.replace(alpha=alpha, gamma=gamma), kinds, f"{kinds.name}, alpha {alpha}, gamma {gamma}, {form}")


def test_beta_zero_is_l1():
    """SMOOTH_L1 with beta 0 (torch: L1): measured against the reference like every SMOOTH_L1 case, and bit for bit the L1 kind's tensors."""
    e = K.make_kind_entry(3300, 2, 5, 67, 7, 40, 12)
    p = CLS_PARAMS[K.CLS_FOCAL]
    devs0 = [T._Dev(e)]
    rows0, sums0 = _run(devs0, p, K.Kinds(K.CLS_FOCAL, K.REG_SMOOTH_L1, 0.0))
    ref0 = K.loss_table([e], p, K.Kinds(K.CLS_FOCAL, K.REG_SMOOTH_L1, 0.0))
    _check(ref0, devs0, rows0, sums0, p, K.Kinds(K.CLS_FOCAL, K.REG_SMOOTH_L1, 0.0), "beta 0")
    devs1 = [T._Dev(e)]
    rows1, _ = _run(devs1, p, K.Kinds(K.CLS_FOCAL, K.REG_L1))
    for a, b in zip(devs0[0].outputs(), devs1[0].outputs()):
        assert torch.equal(a.t.nan_to_num(nan=-7.0), b.t.nan_to_num(nan=-7.0))
    assert bool(((rows0 - rows1).abs() <= 1e-12 * rows1.abs()).all())


@pytest.mark.parametrize("form", [(26, 32, 8), (7, 40, 12)], ids=lambda f: f"{f[0]}cls-ld{f[1]}")
@pytest.mark.parametrize("grad_scale,device_factor", [(-2.5, 1.0), (1.0, 0.125), (-2.5, 0.125)])
def test_backward_factors(grad_scale, device_factor, form):
    """``grad_scale`` and the device-side factor ``sums[n][15]`` enter every gradient once."""
    kinds = K.Kinds(K.CLS_PENALTY_REDUCED, K.REG_HUBER, C)
    e = K.make_kind_entry(3400 + form[0], 2, 5, 67, *form)
    ref, devs, _ = _case([e], CLS_PARAMS[K.CLS_PENALTY_REDUCED], kinds, f"grad_scale {grad_scale}, sums[15] {device_factor}, {form}",
                         grad_scale=grad_scale, device_factor=device_factor)
    plain = K.loss_table([e], CLS_PARAMS[K.CLS_PENALTY_REDUCED], kinds)
    f = R.fp32(grad_scale) * device_factor  # (exact in fp64: the reference's gradients carry the product once)
    assert torch.allclose(ref.entries[0].d_regressands, plain.entries[0].d_regressands * f, rtol=1e-13, atol=0.0)


# ================================================================================================================== entry tables
def _three(seed):
    return [K.make_kind_entry(seed, 2, 8, 300, 26, 32, 32), R.make_entry(seed + 1, 2, 8, 150, 5, 5, 8, empty=True), K.make_kind_entry(seed + 2, 2, 4, 75, 3, 64, 12)]


def _sixteen(seed):
    out = []
    for k in range(16):
        n_cls = 1 + (5 * k) % 7
        ld = (32, n_cls, n_cls + 3)[k % 3]
        if k == 5:
            out.append(R.make_entry(seed + k, 1 + k % 2, 1 + k % 3, 3 + k, n_cls, ld, T.LD_REG[k % 3], instances=2, empty=True))
        else:
            out.append(K.make_kind_entry(seed + k, 1 + k % 2, 1 + k % 3, 3 + k, n_cls, ld, T.LD_REG[k % 3], instances=2))
    return out


@pytest.mark.parametrize("kind", ["three", "sixteen"])
def test_entry_tables(kind):
    """Three entries (one without instances; the global normalisers) and all sixteen lanes of phase two, with the backward scale from the
    totals row."""
    if kind == "three":
        entries, kinds, kw = _three(3500), K.Kinds(K.CLS_PENALTY_REDUCED, K.REG_SMOOTH_L1, C), dict(grad_scale=-2.5, device_factor=0.125)
    else:
        entries, kinds, kw = _sixteen(3530), K.Kinds(K.CLS_FOCAL, K.REG_HUBER, C), dict(device_factor=0.125)
    p = CLS_PARAMS[kinds.cls_kind]
    ref, devs, rows = _case(entries, p, kinds, kind, **kw)
    n = len(entries)
    assert float(rows[n, 12]) == n * float(rows[0, 12]) and float(rows[n, 13]) == n * float(rows[0, 13])
    if kind == "three":
        assert entries[1].num_objects == 0 and float(rows[1, 3]) == 0 and float(rows[0, 3]) > 20 and float(rows[2, 3]) > 20
        assert float(rows[0, 13]) == float(rows[0, 3]) + float(rows[2, 3]) + R.fp32(p.smoothing)


def test_affinity_map_table():
    """PENALTY_REDUCED over affinity maps: the foreground term lives exactly where the MAP is 1 (a tenth of the instance pixels), not
    where the Gaussian of the predictions would be."""
    entries, kinds = _three(3600), K.Kinds(K.CLS_PENALTY_REDUCED, K.REG_MSE)
    maps = [R.make_affinity_map(e, 3610 + k) for k, e in enumerate(entries)]
    inst = entries[0].panoptics > 0
    assert bool((maps[0][inst] == 1).any()) and bool(((maps[0][inst] > 0) & (maps[0][inst] < 1)).any()) and bool((maps[0][inst] == 0).any())
    ref, _, _ = _case(entries, CLS_PARAMS[kinds.cls_kind], kinds, "affinity maps", maps=maps, grad_scale=-2.5, device_factor=0.125)
    assert not torch.equal(K.loss_table(entries, CLS_PARAMS[kinds.cls_kind], kinds).entries[0].foreground, ref.entries[0].foreground)


@pytest.mark.parametrize("aff", [False, True], ids=["plain", "maps"])
def test_default_kinds_are_the_multilevel_pair(aff):
    """kinds {0, 0} through the new pair against the existing pair on the same inputs: tensors bit for bit, sums [0..11] to relative
    1e-12 (the order of the atomic additions), everything else in the rows equal."""
    entries, p = T._three(3700, underflow=True), R.OPTIONS["all"]
    maps = [R.make_affinity_map(e, 3710 + k) for k, e in enumerate(entries)] if aff else [None] * 3
    kw = dict(grad_scale=-2.5, device_factor=0.125)
    old = [T._Dev(e, m) for e, m in zip(entries, maps)]
    rows_old, _ = T._run_table(old, p, **kw)
    new = [T._Dev(e, m) for e, m in zip(entries, maps)]
    rows_new, sums = _run(new, p, K.Kinds(0, 0, float("nan")), **kw)  # (reg_param plays no part in L1)
    assert sums.guard_ok()
    for a, b in zip(old, new):
        for x, y, name in zip(a.outputs(), b.outputs(), ("soft targets", "foreground", "d_logits", "d_regressands")):
            assert torch.equal(x.t.nan_to_num(nan=-7.0), y.t.nan_to_num(nan=-7.0)), name
    assert bool(((rows_new[:, :12] - rows_old[:, :12]).abs() <= 1e-12 * rows_old[:, :12].abs()).all())
    assert torch.equal(rows_new[:, 12:16], rows_old[:, 12:16])
    assert bool(((rows_new[:, 16:] - rows_old[:, 16:]).abs() <= 1e-12 * rows_old[:, 16:].abs()).all())


# ================================================================================================================== refusals
def test_refusals():
    L = _L()
    p = CODING
    e = R.make_entry(3800, 1, 2, 9, 5, 32, 12)
    d = T._Dev(e, R.make_affinity_map(e, 3801))
    sums = T._Buf(2 * R.SUMS_LEN, torch.float64, guard=R.SUMS_LEN)
    outs = list(d.outputs()) + [sums]
    st = L.stream_ptr()
    table, params = (L.LossEntry * 1)(d.struct()), T._params(p)
    maps = (ctypes.c_void_p * 1)(d.aff.data_ptr())
    inf, nan = float("inf"), float("nan")
    bad = [((3, 0, 0.0), "classification kind"), ((-1, 0, 0.0), "classification kind"), ((0, 4, 0.0), "regression kind"), ((0, -1, 0.0), "regression kind"),
           ((1, K.REG_SMOOTH_L1, -0.5), "beta"), ((2, K.REG_HUBER, 0.0), "delta"), ((2, K.REG_HUBER, -1.0), "delta"),
           ((0, K.REG_SMOOTH_L1, nan), "finite"), ((0, K.REG_SMOOTH_L1, inf), "finite"), ((0, K.REG_HUBER, nan), "finite"), ((0, K.REG_HUBER, inf), "finite")]
    for m in (None, maps):
        for (c, r, v), match in bad:
            kk = L.LossKinds(c, r, v)
            T._refused(f"kinds {c, r, v}", "rv_detection_loss_table_forward", (table, 1, ctypes.byref(params), ctypes.byref(kk), m, L.ptr(sums.t), st), outs, match)
            T._refused(f"kinds {c, r, v}", "rv_detection_loss_table_backward", (table, 1, ctypes.byref(params), ctypes.byref(kk), m, L.ptr(sums.t), 1.0, st),
                       outs, match)
        T._refused("null kinds", "rv_detection_loss_table_forward", (table, 1, ctypes.byref(params), None, m, L.ptr(sums.t), st), outs, "null kinds")
        T._refused("null kinds", "rv_detection_loss_table_backward", (table, 1, ctypes.byref(params), None, m, L.ptr(sums.t), 1.0, st), outs, "null kinds")
    ok = L.LossKinds(1, 1, 0.5)
    big = (L.LossEntry * 17)(*[d.struct() for _ in range(17)])
    for n in (0, 17):
        T._refused(f"{n} entries", "rv_detection_loss_table_forward", (big, n, ctypes.byref(params), ctypes.byref(ok), None, L.ptr(sums.t), st), outs, "entries")
        T._refused(f"{n} entries", "rv_detection_loss_table_backward", (big, n, ctypes.byref(params), ctypes.byref(ok), None, L.ptr(sums.t), 1.0, st), outs,
                   "entries")
    no_grad = (L.LossEntry * 1)(d.struct(d_l=False))
    T._refused("null d_logits", "rv_detection_loss_table_backward", (no_grad, 1, ctypes.byref(params), ctypes.byref(ok), None, L.ptr(sums.t), 1.0, st), outs,
               "null gradient")
    null_map = (ctypes.c_void_p * 1)(None)
    T._refused("null map", "rv_detection_loss_table_forward", (table, 1, ctypes.byref(params), ctypes.byref(ok), null_map, L.ptr(sums.t), st), outs, "null affinity map of entry 0")
    T._refused("bad stride", "rv_detection_loss_table_forward", ((L.LossEntry * 1)(d.struct(ld_reg=10)), 1, ctypes.byref(params), ctypes.byref(ok), None, L.ptr(sums.t), st),
               outs, "strides")
