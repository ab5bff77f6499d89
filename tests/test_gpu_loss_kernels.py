"""The fused detection-loss kernels (``csrc/loss.hip``) -- ``rv_detection_loss_forward`` / ``_backward``, the ``_multilevel_`` pair and the
``_multilevel_*_aff`` pair -- against the fp64 reference of ``loss_ref.py``, through the C ABI, on synthetic entries (``loss_ref.make_entry``).

Every output (``d_logits``, ``d_regressands``, soft targets, foreground, sums) is pre-filled with NaN and followed by a guard row that must
keep it; the padding columns of the INPUT rows (``logits[.., n_cls:ld]``, ``regressands[.., 8:ld]``) hold NaN, so a use of them shows
(their values can reach no output; 32-float logits rows are loaded whole, so "never used" is what this proves, not "never read").

EXACT: the foreground map; sums [3], [12], [13], [14] = 0, [15] = 1 (per row and in the totals row, whose [0..11] are 0); in the ``_aff``
form the soft targets, bit for bit the map value at the label; both gradients exactly 0 where ``mask == 0``; ``d_regressands`` exactly 0
where the label is background or ``r == t``; columns ``8..ld_reg-1`` of ``d_regressands`` keep the NaN; the padding columns of ``d_logits``
keep the NaN in the scalar row form and are all zero in the 32-float form (what include/rv3d.h states); guard rows.

ONE fp32 ulp of ``float(reference)``: ``d_regressands`` at ``grad_scale = 1``, ``sums[15] = 1`` (fp64 arithmetic rounded once); one ulp
more per fp32 multiplication with other factors (``grad_scale * (float)sums[15]``, then the product with the gradient).

RELATIVE 1e-12: sums [4..11] and the scalars [20..23] (fp64 sums of fp32-exact terms: only the order of the additions differs).

MEASURED (sums [0..2], scalars [16..19], Gaussian soft targets, ``d_logits``): in fp32 ulps of the size of the terms before they cancel
(``loss_ref`` docstring, UNITS).  The bound is twice the worst figure of the fp32 ORACLE (``oracle.targets.detection_loss``) against the
same reference -- over ``loss_ref.yardstick_cases`` and on the case's own inputs -- and no less than 4 ulp, one ulp more per fp32
multiplication of the backward factors; ``d_logits`` per stratum, and in the tail stratum (negatives with x < -2, where the fp32 oracle's own BCE cancels and is no yardstick:
tests/test_loss_ref_cpu.py) ``loss_ref.TAIL_ULP``, from the precision of the formats.  Worst figures (oracle: an x86-64 host, over the
yardstick cases; kernel: an MI355X, over every case of this module -- ``pytest -s`` prints them):

    quantity                         fp32 oracle (CPU)   bound >= kernel (MI355X)
    sums [0..2]                      (as the scalars)    4        1.28
    scalars [16..19]                 1.63                4        1.51
    soft targets (Gaussian)          13.8                27.7     20.4
    d_logits, positives              20.7                41.5     24.8
    d_logits, negatives x >= -2      18.4                36.8     21.0
    d_logits, negatives x < -2       9.72e6              40       10.2
    d_regressands                    (not measured)      1 (+1 per fp32 multiplication)   1.0

The "bound >=" column is what the yardstick cases alone give: a FLOOR of the asserted limit.  The oracle's figure on a case's own inputs
raises the limit of that case where it is the larger one (the two cases of 131 200 and 524 800 pixels, the tables), and the backward
factors add their one or two ulp.  The largest limits applied over the module (printed next to the worst figures):
sums / scalars 15.4 (the fp32 oracle sums half a million pixels in fp32), soft targets 40.8, d_logits 58.5 / 41.7 / 42 (with two factors).

Mechanism -> case:

* both class loops of ``loss_tile`` (32-float rows: unrolled 16-byte form; every other row length: scalar), every lane of ``lv`` / ``gv``,
  ``ld_reg`` 8 / 12 / 32, a ragged last workgroup and three idle waves ............................. test_one_entry_row_forms
* every hyper-parameter one at a time and all together, the ``powf`` branch, ``az_inv = 0``, underflow of the affinity at sigma 0.25,
  smoothing 0 ..................................................................................... test_options
* ``grad_scale`` and the device-side factor ``sums[15]`` ........................................... test_backward_factors
* no instance (normaliser 1), mask all zero ......................................................... test_empty_cases
* grid-stride beyond the forward cap (512 workgroups) and the backward cap (2048) ................... test_grid_stride
* the entry table: ``block_begin`` after a large entry, an entry without instances, all 16 lanes of ``loss_table_finish_kernel``, the
  global normalisers and the totals row, the backward scale from the totals row ..................... test_entry_tables
* affinity read from a map .......................................................................... test_affinity_maps
* refusals ........................................................................................... test_refusals

The module was run on an MI355X against six builds of ``loss.hip`` with one value-only mutation each; every one was caught (the id
named is one of those that failed, with the assertion that failed first in it):

* ``coding[j]`` -> ``coding[7 - j]`` (both uses): 21 failed .... test_options[coding-26cls-ld32], [20..23] at relative 1e-12
* ``powf(p, gamma)`` -> ``p * p``: 15 failed ................... test_options[gamma_1.5-26cls-ld32], sums [0..2] off by 2.7e5 ulp
* ``lv[c >> 2][c & 3]`` -> ``[(c + 1) & 3]``: 54 failed, every case with 32-float rows and none other
  ............................................................. test_one_entry_row_forms[3cls-ld32-2x5x67], sums [0..2] not finite
* ``* m`` dropped from the logits gradient: 73 failed, all but six tiny cases without a masked pixel
  ............................................................. test_one_entry_row_forms[26cls-ld32-2x5x67], d_logits
* ``az_inv`` ignored (always 1): 7 failed ...................... test_options[az_inv_0-26cls-ld32], sums [0..2] off by 5.9e5 ulp
* phase two with the entry's own ``s[3]``: 6 failed, every table of more than one entry
  ............................................................. test_entry_tables[three], row 0 [13] = 276, expected 414
"""

from __future__ import annotations

import ctypes
import math

import pytest
import torch

import loss_ref as R
from test_gpu_forward import DEV

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
WORST = {}  # worst measured figure per quantity over the module (printed at teardown)
APPLIED = {}  # largest bound applied per quantity over the module (the case's own inputs can raise it over the yardstick cases')


def _L():
    from range_view_3d_detection_amd import _lib as L

    return L


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nloss kernels vs loss_ref, worst fp32 ulps: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items()))
              + "; bounds from the yardstick cases: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(R.kernel_bounds().items()))
              + "; largest bound applied: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(APPLIED.items())))


class _Buf:
    """An output of n elements, NaN-filled, followed by a guard row."""

    def __init__(self, n, dtype=torch.float32, guard=GUARD):
        self.n = n
        self.t = torch.full((n + guard,), NAN, dtype=dtype, device=DEV)

    def body(self, *shape):
        return self.t[:self.n].view(*shape).cpu()

    def guard_ok(self):
        return bool(self.t[self.n:].isnan().all())

    def untouched(self):
        return bool(self.t.isnan().all())


class _Dev:
    """One entry on the device: its inputs, its sentinel-filled outputs."""

    def __init__(self, e: R.Entry, aff=None):
        self.e = e
        B, H, W = e.shape
        px = B * H * W
        self.inp = [t.to(DEV).contiguous() for t in (e.logits, e.regressands, e.cart, e.mask, e.labels, e.panoptics, e.reg_targets, e.points_per_obj)]
        self.nobj = torch.tensor([e.num_objects], dtype=torch.int32, device=DEV)
        self.aff = None if aff is None else aff.to(DEV).contiguous()
        self.soft, self.fg = _Buf(px * e.n_cls), _Buf(px)
        self.d_l, self.d_r = _Buf(px * e.ld_logits, guard=max(GUARD, e.ld_logits)), _Buf(px * e.ld_reg, guard=max(GUARD, e.ld_reg))

    def outputs(self):
        return (self.soft, self.fg, self.d_l, self.d_r)

    def struct(self, ld_logits=None, ld_reg=None, d_l=True):
        L, e = _L(), self.e
        B, H, W = e.shape
        return L.LossEntry(*[t.data_ptr() for t in self.inp], self.nobj.data_ptr(), self.soft.t.data_ptr(), self.fg.t.data_ptr(),
                           self.d_l.t.data_ptr() if d_l else None, self.d_r.t.data_ptr(), ld_logits or e.ld_logits, ld_reg or e.ld_reg, B, e.n_cls, H, W)

    def one_level_args(self, p, ld_logits=None, ld_reg=None):
        L, e = _L(), self.e
        B, H, W = e.shape
        lg, rg, rest = self.inp[0], self.inp[1], self.inp[2:]
        self.coding = (ctypes.c_float * 8)(*[float(c) for c in p.coding_weights])
        return (L.ptr(lg), ld_logits or e.ld_logits, L.ptr(rg), ld_reg or e.ld_reg, *[L.ptr(t) for t in rest], L.ptr(self.nobj),
                B, e.n_cls, H, W, self.coding, p.cls_weight, p.reg_weight, p.smoothing, p.sigma,
                p.alpha, p.gamma, 1 if p.az_inv else 0)


def _params(p):
    L = _L()
    return L.LossParams((ctypes.c_float * 8)(*[float(c) for c in p.coding_weights]), p.cls_weight, p.reg_weight, p.smoothing, p.sigma, p.alpha, p.gamma,
                        1 if p.az_inv else 0)


def _run_one(d: _Dev, p, grad_scale=1.0, device_factor=1.0):
    """The one-level pair; returns (rows (1, 24) as forward left them, the sums buffer)."""
    L = _L()
    sums = _Buf(R.SUMS_LEN, torch.float64, guard=R.SUMS_LEN)
    args = d.one_level_args(p)
    L.call("rv_detection_loss_forward", *args, L.ptr(sums.t), L.ptr(d.soft.t), L.ptr(d.fg.t), L.stream_ptr())
    torch.cuda.synchronize()
    rows = sums.body(1, R.SUMS_LEN)
    if device_factor != 1.0:
        sums.t[15] = device_factor
    L.call("rv_detection_loss_backward", *args, L.ptr(sums.t), grad_scale, L.ptr(d.d_l.t), L.ptr(d.d_r.t), L.stream_ptr())
    torch.cuda.synchronize()
    return rows, sums


def _run_table(devs, p, grad_scale=1.0, device_factor=1.0):
    """The multi-level pair, or the ``_aff`` pair when the entries carry maps; returns (rows (n + 1, 24), the sums buffer)."""
    L, n = _L(), len(devs)
    sums = _Buf((n + 1) * R.SUMS_LEN, torch.float64, guard=R.SUMS_LEN)
    table = (L.LossEntry * n)(*[d.struct() for d in devs])
    params = _params(p)
    aff = devs[0].aff is not None
    maps = (ctypes.c_void_p * n)(*[d.aff.data_ptr() for d in devs]) if aff else None
    tail = (L.ptr(sums.t),)
    if aff:
        L.call("rv_detection_loss_multilevel_forward_aff", table, n, ctypes.byref(params), maps, *tail, L.stream_ptr())
    else:
        L.call("rv_detection_loss_multilevel_forward", table, n, ctypes.byref(params), *tail, L.stream_ptr())
    torch.cuda.synchronize()
    rows = sums.body(n + 1, R.SUMS_LEN)
    if device_factor != 1.0:
        sums.t[n * R.SUMS_LEN + 15] = device_factor
    if aff:
        L.call("rv_detection_loss_multilevel_backward_aff", table, n, ctypes.byref(params), maps, *tail, grad_scale, L.stream_ptr())
    else:
        L.call("rv_detection_loss_multilevel_backward", table, n, ctypes.byref(params), *tail, grad_scale, L.stream_ptr())
    torch.cuda.synchronize()
    return rows, sums


def _measured(fig, bounds, extra, what):
    for k, v in fig.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(fig.items())))
    for k, v in fig.items():
        more = extra if k.startswith("d_logits") else 0
        APPLIED[k] = max(APPLIED.get(k, 0.0), bounds[k] + more)
        assert v <= bounds[k] + more, f"{what}: {k} is off by {v:.4g} fp32 ulp (bound {bounds[k] + more:.4g})"


def _rel12(got, ref, what):
    assert bool(((got - ref).abs() <= 1e-12 * ref.abs()).all()), f"{what}: {got.tolist()} vs {ref.tolist()}"


def _check(ref: R.TableResult, devs, rows, sums, p, what, grad_scale=1.0, device_factor=1.0, totals=True):
    """Everything the module docstring lists, for the outputs of one forward + backward over ``devs``."""
    n = len(devs)
    # the yardstick on the same inputs: the fp32 oracle on every entry (it takes no affinity map: the ``_aff`` form keeps the yardstick cases')
    own = [R.oracle_fp32_figures(d.e, p) if d.aff is None else {} for d in devs]
    per_entry = [R.kernel_bounds(f) for f in own]
    bounds = R.kernel_bounds({k: max(f.get(k, 0.0) for f in own) for k in R.MEASURED})
    # one ulp more per fp32 multiplication: grad_scale * (float)sums[15] rounds when both differ from 1, the product with the gradient when either does
    extra = int(grad_scale != 1.0 or device_factor != 1.0) + int(grad_scale != 1.0 and device_factor != 1.0)
    assert sums.guard_ok(), f"{what}: wrote behind the sums"
    for k in range(n + (1 if totals else 0)):
        got, want = rows[k], ref.rows[k]
        for j in (3, 12, 13, 14, 15):
            assert float(got[j]) == float(want[j]), f"{what}: row {k} [{j}] = {float(got[j])!r}, expected {float(want[j])!r}"
        _rel12(got[20:24], want[20:24], f"{what}: row {k} [20..23]")
        if k < n:
            _rel12(got[4:12], want[4:12], f"{what}: row {k} [4..11]")
        else:
            assert bool((got[:12] == 0).all()), f"{what}: totals row [0..11]"
        _measured(R.figures(ref, k, row={j: float(got[j]) for j in ((0, 1, 2) if k < n else ()) + (16, 17, 18, 19)}), bounds, 0, f"{what} row {k}")
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
            assert torch.equal(er.foreground, (amap != 0).double())
            fig = R.figures(ref, k, d_logits=d_l[..., :n_cls])
        else:
            fig = R.figures(ref, k, soft=soft, d_logits=d_l[..., :n_cls])
        _measured(fig, per_entry[k], extra, w)
        # padding columns
        assert bool(d_r[..., 8:].isnan().all()), f"{w}: columns 8.. of d_regressands were written"
        if row32:
            assert bool((d_l[..., n_cls:] == 0).all()), f"{w}: padding columns of d_logits (32-float rows) are not all zero"
        else:
            assert bool(d_l[..., n_cls:].isnan().all()), f"{w}: padding columns of d_logits (scalar form) were written"
        # exact zeros
        off = e.mask == 0
        assert bool((d_l[..., :n_cls][off] == 0).all()) and bool((d_r[..., :8][off] == 0).all()), f"{w}: gradient where mask == 0"
        g_r, want_r = d_r[..., :8].double(), er.d_regressands
        r_is_t = e.regressands[..., :8] == e.reg_targets.permute(0, 2, 3, 1)
        zero = (e.labels == n_cls)[..., None] | r_is_t | off[..., None]
        assert bool((want_r[zero] == 0).all()) and bool((want_r[~zero] != 0).all())
        assert bool((g_r[zero] == 0).all()), f"{w}: d_regressands where the label is background or r == t"
        err = (g_r - want_r.float().double()).abs() / R.ulp32(want_r)
        worst = float(torch.nan_to_num(err, nan=math.inf).max())
        WORST["d_regressands"] = max(WORST.get("d_regressands", 0.0), worst)
        assert worst <= 1 + extra, f"{w}: d_regressands is off by {worst:.3g} fp32 ulp (allowed {1 + extra})"


def _one(e, p, what, **kw):
    d = _Dev(e)
    rows, sums = _run_one(d, p, **kw)
    ref = R.loss_one(e, p, **kw)
    _check(ref, [d], rows, sums, p, what, totals=False, **kw)
    return ref, d, rows


# ================================================================================================================== one entry
ROW32 = [1, 3, 4, 5, 26, 31, 32]
FORMS = [(n, 32) for n in ROW32] + [(3, 3), (7, 40), (33, 64)]
LD_REG = (8, 12, 32)


@pytest.mark.parametrize("dims", [(2, 5, 67), (1, 1, 5)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("i", range(len(FORMS)), ids=[f"{n}cls-ld{ld}" for n, ld in FORMS])
def test_one_entry_row_forms(i, dims):
    """Both class loops at every class count that ends a 16-byte group differently; 2x5x67 = 670 pixels: three workgroups, the last one
    ragged; 1x1x5: one wave with five lanes, three waves idle (they still take part in the workgroup's reduction)."""
    n_cls, ld = FORMS[i]
    ld_reg = LD_REG[(i + (dims[0] == 1)) % 3]
    e = R.make_entry(300 + i, *dims, n_cls, ld, ld_reg)
    ref, _, _ = _one(e, R.DEFAULT, f"{n_cls} classes, ld {ld}, ld_reg {ld_reg}, {dims}")
    if dims[0] == 2:
        assert int(ref.rows[0, 3]) > 20 and bool((e.mask == 0)[e.panoptics > 0].any())


@pytest.mark.parametrize("form", [(26, 32, 8), (3, 32, 32), (7, 40, 12)], ids=lambda f: f"{f[0]}cls-ld{f[1]}")
@pytest.mark.parametrize("name", list(R.OPTIONS))
def test_options(name, form):
    p = R.OPTIONS[name]
    quarter = R.fp32(p.sigma) == 0.25
    e = R.make_entry(500 + form[0], 2, 5, 67, *form, underflow=quarter)
    ref, _, _ = _one(e, p, f"{name}, {form}")
    er = ref.entries[0]
    assert int(ref.rows[0, 3]) > 20, "no foreground"
    if quarter:  # instance pixels whose affinity underflows are not foreground
        far = e.planted["far"]
        assert int(far.sum()) >= 3 and bool((er.foreground[far] == 0).all())
    if p.az_inv:
        assert bool((er.soft.sum(1)[e.planted["exact"]] == 1.0).all())


@pytest.mark.parametrize("form", [(26, 32, 8), (7, 40, 12)], ids=lambda f: f"{f[0]}cls-ld{f[1]}")
@pytest.mark.parametrize("grad_scale,device_factor", [(-2.5, 1.0), (1.0, 0.125), (-2.5, 0.125)])
def test_backward_factors(grad_scale, device_factor, form):
    e = R.make_entry(600 + form[0], 2, 5, 67, *form)
    _one(e, R.OPTIONS["coding"], f"grad_scale {grad_scale}, sums[15] {device_factor}, {form}", grad_scale=grad_scale, device_factor=device_factor)


@pytest.mark.parametrize("form", [(3, 32, 8), (5, 5, 12)], ids=lambda f: f"{f[0]}cls-ld{f[1]}")
@pytest.mark.parametrize("kind", ["no_instance", "mask_zero"])
def test_empty_cases(kind, form):
    e = R.make_entry(700 + form[0], 2, 5, 67, *form, empty=kind == "no_instance", mask_zero=kind == "mask_zero")
    ref, d, rows = _one(e, R.OPTIONS["coding"], f"{kind}, {form}")
    if kind == "no_instance":
        assert e.num_objects == 0 and float(rows[0, 12]) == 1.0 and float(rows[0, 3]) == 0.0 and float(rows[0, 13]) == 1.0
        assert bool((d.d_r.body(2, 5, 67, e.ld_reg)[..., :8] == 0).all()) and float(rows[0, 23]) == 0.0
    else:
        assert float(rows[0, 3]) > 20 and float(rows[0, 16]) == 0.0 and bool((rows[0, :3] == 0).all())
        assert bool((d.d_l.body(2, 5, 67, e.ld_logits)[..., :e.n_cls] == 0).all())


GRID_FWD, GRID_BWD = (2, 8, 8200), (1, 8, 65600)


@pytest.mark.parametrize("dims", [GRID_FWD, GRID_BWD], ids=lambda d: "x".join(map(str, d)))
def test_grid_stride(dims):
    """131 200 pixels > 512 workgroups x 256 (the forward pass's second sweep is ragged: 128 pixels, an instance among them);
    524 800 > 2048 x 256 for the backward pass.  32-float rows, 3 classes."""
    B, H, W = dims
    assert B * H * W > (131072 if dims == GRID_FWD else 524288)
    e = R.make_entry(800 + B, B, H, W, 3, 32, 8, instances=12)
    assert bool((e.panoptics[-1, -1, -40:] > 0).all())
    _one(e, R.OPTIONS["coding"], f"grid-stride {dims}")


# ================================================================================================================== entry tables
def _three(seed, underflow=False):
    return [R.make_entry(seed, 2, 8, 300, 26, 32, 32, underflow=underflow), R.make_entry(seed + 1, 2, 8, 150, 5, 5, 8, empty=True),
            R.make_entry(seed + 2, 2, 4, 75, 3, 64, 12, underflow=underflow)]


def _sixteen(seed):
    """16 entries of distinct tiny shapes, both row forms: every lane of the finish kernel."""
    out = []
    for k in range(16):
        n_cls = 1 + (5 * k) % 7
        ld = (32, n_cls, n_cls + 3)[k % 3]
        out.append(R.make_entry(seed + k, 1 + k % 2, 1 + k % 3, 3 + k, n_cls, ld, LD_REG[k % 3], instances=2, empty=k == 5))
    return out


def _table(entries, p, what, **kw):
    devs = [_Dev(e) for e in entries]
    rows, sums = _run_table(devs, p, **kw)
    ref = R.loss_table(entries, p, **kw)
    _check(ref, devs, rows, sums, p, what, **kw)
    n = len(entries)
    assert float(rows[n, 12]) == n * float(rows[0, 12]) and float(rows[n, 13]) == n * float(rows[0, 13])
    return ref, devs, rows


@pytest.mark.parametrize("kind", ["three", "three_all_options", "large_then_tiny", "sixteen", "one"])
def test_entry_tables(kind):
    if kind == "three":
        entries, p, kw = _three(900), R.OPTIONS["coding"], {}
    elif kind == "three_all_options":  # and the backward scale from the totals row's [15]
        entries, p, kw = _three(910, underflow=True), R.OPTIONS["all"], dict(grad_scale=-2.5, device_factor=0.125)
    elif kind == "large_then_tiny":  # 512 forward workgroups in front of a one-workgroup entry
        entries, p, kw = [R.make_entry(920, *GRID_FWD, 3, 32, 8, instances=12), R.make_entry(921, 1, 1, 5, 4, 32, 12)], R.OPTIONS["coding"], {}
    elif kind == "sixteen":
        entries, p, kw = _sixteen(930), R.OPTIONS["coding"], dict(device_factor=0.125)
    else:
        entries, p, kw = [R.make_entry(950, 2, 5, 67, 26, 32, 8)], R.OPTIONS["coding"], {}
    ref, devs, rows = _table(entries, p, kind, **kw)
    if kind.startswith("three"):
        assert entries[1].num_objects == 0 and float(rows[1, 3]) == 0 and float(rows[0, 3]) > 20 and float(rows[2, 3]) > 20
        assert float(rows[0, 13]) == float(rows[0, 3]) + float(rows[2, 3]) + R.fp32(p.smoothing)  # the GLOBAL count, not the entry's own
    if kind == "one":  # "with one entry every tensor and row 0 equal the one-level entry points' results"
        d = _Dev(entries[0])
        rows1, _ = _run_one(d, p)
        for a, b in zip(devs[0].outputs(), d.outputs()):
            assert torch.equal(a.t.nan_to_num(nan=-7.0), b.t.nan_to_num(nan=-7.0))
        assert bool(((rows[0] - rows1[0]).abs() <= 1e-12 * rows1[0].abs()).all())


@pytest.mark.parametrize("kw", [{}, dict(grad_scale=-2.5, device_factor=0.125)], ids=["plain", "factors"])
def test_affinity_maps(kw):
    """Foreground, soft targets and gradients follow the MAP (0 off-instance, 0 on some instance pixels, exactly 1 on some), not the Gaussian
    of the predictions -- which, with sigma 0.25 and the underflow pixels, would give another foreground."""
    entries, p = _three(960, underflow=True), R.OPTIONS["all"]
    maps = [R.make_affinity_map(e, 970 + k) for k, e in enumerate(entries)]
    devs = [_Dev(e, m) for e, m in zip(entries, maps)]
    rows, sums = _run_table(devs, p, **kw)
    ref = R.loss_table(entries, p, aff_maps=maps, **kw)
    _check(ref, devs, rows, sums, p, "affinity maps", **kw)
    gauss = R.loss_table(entries, p)
    inst = entries[0].panoptics > 0
    assert not torch.equal(gauss.entries[0].foreground, ref.entries[0].foreground)
    assert bool((maps[0][inst] == 0).any()) and bool((maps[0][inst] == 1).any()) and bool((maps[0][~inst] == 0).all())


# ================================================================================================================== refusals
def _refused(fn, name, args, outs, match):
    L = _L()
    with pytest.raises(L.RvError, match=match) as info:
        L.call(name, *args)
    assert len(str(info.value)) > len(name) + 10
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched(), f"{fn}: the refused call wrote an output"


def test_refusals():
    L = _L()
    p = R.OPTIONS["coding"]
    e = R.make_entry(990, 1, 2, 9, 5, 32, 12)
    d = _Dev(e, R.make_affinity_map(e, 991))
    sums = _Buf(2 * R.SUMS_LEN, torch.float64, guard=R.SUMS_LEN)
    outs = list(d.outputs()) + [sums]
    st = L.stream_ptr()
    fwd_tail, bwd_tail = (L.ptr(sums.t), L.ptr(d.soft.t), L.ptr(d.fg.t), st), (L.ptr(sums.t), 1.0, L.ptr(d.d_l.t), L.ptr(d.d_r.t), st)
    for what, kw, match in (("ld_logits < n_cls", dict(ld_logits=4), "strides"), ("ld_reg = 10", dict(ld_reg=10), "strides")):
        _refused(what, "rv_detection_loss_forward", d.one_level_args(p, **kw) + fwd_tail, outs, match)
        _refused(what, "rv_detection_loss_backward", d.one_level_args(p, **kw) + bwd_tail, outs, match)
        table = (L.LossEntry * 1)(d.struct(**kw))
        _refused(what, "rv_detection_loss_multilevel_forward", (table, 1, ctypes.byref(_params(p)), L.ptr(sums.t), st), outs, match)
        _refused(what, "rv_detection_loss_multilevel_backward", (table, 1, ctypes.byref(_params(p)), L.ptr(sums.t), 1.0, st), outs, match)
    _refused("null d_logits", "rv_detection_loss_backward", d.one_level_args(p) + (L.ptr(sums.t), 1.0, None, L.ptr(d.d_r.t), st), outs, "null gradient")
    _refused("null d_regressands", "rv_detection_loss_backward", d.one_level_args(p) + (L.ptr(sums.t), 1.0, L.ptr(d.d_l.t), None, st), outs, "null gradient")
    table = (L.LossEntry * 17)(*[d.struct() for _ in range(17)])
    maps = (ctypes.c_void_p * 17)(*[d.aff.data_ptr()] * 17)
    params = _params(p)
    for n in (0, 17):
        _refused(f"{n} entries", "rv_detection_loss_multilevel_forward", (table, n, ctypes.byref(params), L.ptr(sums.t), st), outs, "entries")
        _refused(f"{n} entries", "rv_detection_loss_multilevel_backward", (table, n, ctypes.byref(params), L.ptr(sums.t), 1.0, st), outs, "entries")
        _refused(f"{n} entries", "rv_detection_loss_multilevel_forward_aff", (table, n, ctypes.byref(params), maps, L.ptr(sums.t), st), outs, "entries")
        _refused(f"{n} entries", "rv_detection_loss_multilevel_backward_aff", (table, n, ctypes.byref(params), maps, L.ptr(sums.t), 1.0, st), outs, "entries")
    no_grad = (L.LossEntry * 1)(d.struct(d_l=False))
    _refused("null d_logits in the table", "rv_detection_loss_multilevel_backward", (no_grad, 1, ctypes.byref(params), L.ptr(sums.t), 1.0, st), outs, "null gradient")
    _refused("null d_logits in the table", "rv_detection_loss_multilevel_backward_aff", (no_grad, 1, ctypes.byref(params), maps, L.ptr(sums.t), 1.0, st), outs,
             "null gradient")
    null_map = (ctypes.c_void_p * 1)(None)
    for m, match in ((None, "null affinity maps"), (null_map, "null affinity map of entry 0")):
        _refused("null map", "rv_detection_loss_multilevel_forward_aff", (table, 1, ctypes.byref(params), m, L.ptr(sums.t), st), outs, match)
        _refused("null map", "rv_detection_loss_multilevel_backward_aff", (table, 1, ctypes.byref(params), m, L.ptr(sums.t), 1.0, st), outs, match)
