"""The fused detection loss (``csrc/loss.hip``: ``rv_detection_loss_forward`` / ``_backward``, the ``_multilevel_`` pair and the
``_multilevel_*_aff`` pair) restated in plain torch on the CPU, in fp64, from the documented operation: the comments of
``include/rv3d.h`` on the three families, ``oracle/targets.py`` (``classification_targets``, ``varifocal_loss``, ``detection_loss``) and
phase two as ``rv3d.h`` describes it (``reduce_multiscale_loss``).  TEST INFRASTRUCTURE: tests/test_loss_ref_cpu.py pins it to the
fixtures and to the oracle; tests/test_gpu_loss_kernels.py compares the kernels with it.

The operation, per (level, task) ENTRY and pixel (all arithmetic fp64 unless said otherwise):

* centres: ``decode_range_view`` of the prediction (always azimuth-invariant) and of the target (``az_inv``), fp64 ROUNDED TO fp32
  (the operation is defined so: the decoder returns the dtype of its input);
* affinity: ``a = exp(-||c_pred - c_target|| / sigma^2)`` on instance pixels (``panoptics > 0``), 0 elsewhere.  The soft targets are
  fp32 tensors: an affinity that rounds to 0 in fp32 IS 0 (the pixel is an instance pixel that is not foreground).  In the ``_aff``
  form ``a`` is read from the given map instead.  foreground = ``a != 0``, background = ``!foreground & mask``;
* soft target ``t[c] = a`` at ``c == label``, else 0 (detached: no gradient flows into the affinity);
* classification: ``VFL = t > 0 ? t * (softplus(x) - x t) : alpha * sigmoid(x)^gamma * softplus(x)``; ``cls = cls_weight * VFL * mask``;
  sums[0] = sum cls, [1] = over foreground, [2] = over background, [3] = #foreground;
* regression, on pixels with ``label < n_cls``: ``(|r - t| * reg_weight)`` IN fp32 (the L1 loss and its weight are fp32 tensors), then
  fp64: ``* 1 / (points_per_obj + smoothing) * mask * coding_weights[j] / 8``; sums[4 + j] = the sum for regressand j;
* phase two over the table: ``total_fg = sum_e sums_e[3] + smoothing``, ``total_objects = max(sum_e num_objects_e, 1)``; row e
  [12] = total_objects, [13] = total_fg, [14] = 0, [15] = 1, [16..23] = loss, classification, foreground, background, coordinate,
  dimension, rotation, regression -- every one normalised by the two GLOBAL numbers; the totals row = [16..23] summed over the
  entries, [12] / [13] = n x the global numbers, [15] = 1, [0..11] = 0.  A table of one entry is the one-level entry point's row.
* gradients: AUTOGRAD through this fp64 forward of ``totals[16] * grad_scale * sums[15]`` (the two factors as the fp32 / fp64 numbers
  the kernel receives).  Where the forward value is defined in fp32 (``|r - t| * reg_weight``) the value is the fp32 one and the
  gradient flows through the same expression in fp64 (a straight-through term of value 0).

Every hyper-parameter enters as the fp32 number the C ABI carries.

UNITS of the measured comparisons (``figures``): errors are counted in fp32 ulps of the SIZE of the terms before they cancel, with a
floor of the smallest normal fp32 on the size:

* a soft target: its own value;
* an element of ``d_logits``: ``cls_weight |scale| / total_fg * t * max(p, t)`` on a positive (``t (p - t)`` cancels), its own value on
  a negative (a product of positive factors);
* sums[0..2]: the sum over the pixels it covers of ``cls_weight * mask * (t > 0 ? t * max(softplus(x), |x| t) : VFL)``
  (``softplus(x) - x t`` cancels); the classification scalars [17..19]: that / total_fg; the loss [16]: that of [17] + the regression loss.

The synthetic entries (``make_entry``) are drawn without any target kernel, see there.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

FLT_MIN = 2.0 ** -126
SUMS_LEN = 24
NAN = float("nan")


def fp32(v: float) -> float:
    """The fp32 number the C ABI carries for a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


@dataclass
class Params:
    """``rvLossParams``."""

    coding_weights: Sequence[float] = (1.0,) * 8
    cls_weight: float = 1.0
    reg_weight: float = 1.0
    smoothing: float = 1.0
    sigma: float = 0.75
    alpha: float = 0.75
    gamma: float = 2.0
    az_inv: bool = True

    def replace(self, **kw) -> "Params":
        d = dict(self.__dict__)
        d.update(kw)
        return Params(**d)


@dataclass
class Entry:
    """One (level, task) as the C ABI takes it: logits / regressands NHWC fp32 WITH their padding columns (NaN), cart / reg_targets NCHW
    fp32, mask u8, labels / panoptics / points_per_obj i64 (B,H,W)."""

    logits: torch.Tensor        # (B,H,W,ld_logits)
    regressands: torch.Tensor   # (B,H,W,ld_reg)
    cart: torch.Tensor          # (B,3,H,W)
    mask: torch.Tensor          # (B,H,W) u8
    labels: torch.Tensor
    panoptics: torch.Tensor
    reg_targets: torch.Tensor   # (B,8,H,W)
    points_per_obj: torch.Tensor
    num_objects: int
    n_cls: int
    planted: Dict[str, torch.Tensor] = field(default_factory=dict)  # what make_entry planted (bool maps), for the tests' own checks

    @property
    def shape(self):
        return tuple(self.labels.shape)

    @property
    def ld_logits(self) -> int:
        return int(self.logits.shape[-1])

    @property
    def ld_reg(self) -> int:
        return int(self.regressands.shape[-1])


@dataclass
class EntryResult:
    soft: torch.Tensor        # (B,n_cls,H,W) f64
    foreground: torch.Tensor  # (B,H,W) f64 in {0, 1}
    d_logits: torch.Tensor    # (B,H,W,n_cls) f64
    d_regressands: torch.Tensor  # (B,H,W,8) f64
    size_d_logits: torch.Tensor  # (B,H,W,n_cls) f64: the unit of the measured comparison
    stratum: torch.Tensor     # (B,H,W,n_cls) i64: 0 = positive (t > 0), 1 = negative with x >= TAIL_X, 2 = negative with x < TAIL_X
    affinity_arg: Optional[torch.Tensor]  # (B,H,W) d / sigma^2 on instance pixels (Gaussian form), else None


@dataclass
class TableResult:
    rows: torch.Tensor   # (n + 1, 24) f64
    sizes: torch.Tensor  # (n + 1, 24) f64: the unit of [0], [1], [2], [16..19]; NaN elsewhere
    entries: List[EntryResult]


def ulp32(size: torch.Tensor) -> torch.Tensor:
    """The fp32 unit in the last place at |size| (fp64), the size floored at the smallest normal fp32."""
    s = size.detach().abs().double().clamp_min(FLT_MIN)
    _, e = torch.frexp(s)
    return torch.ldexp(torch.ones_like(s), e - 24)


def decode_centre(r: torch.Tensor, cart: torch.Tensor, az_inv: bool) -> torch.Tensor:
    """(B,8,H,W) fp32 regressands + (B,3,H,W) fp32 points -> (B,3,H,W): fp64 arithmetic rounded to fp32, returned as fp64 numbers."""
    p, dx, dy = cart.double(), r[:, 0].double(), r[:, 1].double()
    if az_inv:
        az = torch.atan2(p[:, 1], p[:, 0])
        s, c = az.sin(), az.cos()
        dx, dy = c * dx - s * dy, s * dx + c * dy
    return torch.stack([p[:, 0] + dx, p[:, 1] + dy, p[:, 2] + r[:, 2].double()], dim=1).float().double()


def gaussian_affinity(e: Entry, p: Params):
    """(affinity (B,H,W) f64 with the fp32 zeros, d / sigma^2 (B,H,W) f64)."""
    r = e.regressands[..., :8].permute(0, 3, 1, 2)
    sigma = fp32(p.sigma)
    d = (decode_centre(r, e.cart, True) - decode_centre(e.reg_targets, e.cart, bool(p.az_inv))).norm(dim=1)
    u = d / fp32(sigma * sigma)
    inst = e.panoptics > 0
    band = inst & (u > 60.0) & (u < 125.0)
    assert not bool(band.any()), "an instance pixel with d / sigma^2 in (60, 125): fp32 exponentials may differ in denormal handling there"
    a = torch.exp(-u) * inst
    return torch.where(a.float() == 0, torch.zeros_like(a), a), u


def _softplus(x):
    """log(1 + e^x) in fp64, smooth at 0 for autograd (max(x, 0) + log1p(e^-|x|) has the sub-gradient 1 there instead of 1/2) and without
    torch's default cut at x > 20, which costs e^-20 in fp64; |x| stays far below the overflow of e^x."""
    assert float(x.detach().abs().max()) < 500.0
    return torch.nn.functional.softplus(x, beta=1.0, threshold=1000.0)


def _entry_forward(e: Entry, p: Params, aff_map: Optional[torch.Tensor]):
    n = e.n_cls
    x = e.logits[..., :n].permute(0, 3, 1, 2).double().clone().requires_grad_(True)
    r32 = e.regressands[..., :8].permute(0, 3, 1, 2).contiguous()
    r = r32.double().clone().requires_grad_(True)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(r).all())
    m = (e.mask != 0).double()[:, None]
    if aff_map is None:
        aff, u = gaussian_affinity(e, p)
    else:
        aff, u = aff_map.double(), None
    fg = aff != 0
    bg = (~fg) & (e.mask != 0)
    one_hot = e.labels[:, None] == torch.arange(n).view(1, n, 1, 1)
    t = aff[:, None] * one_hot
    pos = t > 0
    sp, prob = _softplus(x), torch.sigmoid(x)
    alpha, gamma, cls_w = fp32(p.alpha), fp32(p.gamma), fp32(p.cls_weight)
    vfl = torch.where(pos, t * (sp - x * t), alpha * prob.pow(gamma) * sp)
    cls = cls_w * vfl * m
    size = (cls_w * m * torch.where(pos, t * torch.maximum(sp, x.abs() * t), vfl)).detach()
    s = [cls.sum(), (cls * fg[:, None]).sum(), (cls * bg[:, None]).sum(), fg.sum().double()]
    sizes = [size.sum(), (size * fg[:, None]).sum(), (size * bg[:, None]).sum()]
    # regression
    smoothing, reg_w = fp32(p.smoothing), fp32(p.reg_weight)
    on = e.labels < n  # (off these pixels points_per_obj is 0 and, with smoothing 0, the normaliser is not defined: they take no part)
    norm = torch.where(on, 1.0 / (e.points_per_obj.double() + smoothing).where(on, torch.ones(())), torch.zeros(()).double())[:, None]
    l1_32 = ((r32 - e.reg_targets).abs() * torch.tensor(reg_w, dtype=torch.float32)).double()  # the fp32 tensors of the operation
    l1_64 = (r - e.reg_targets.double()).abs() * reg_w
    l1 = l1_32 + (l1_64 - l1_64.detach())  # value: fp32-defined; gradient: through the fp64 expression
    coding = torch.tensor([fp32(c) for c in p.coding_weights], dtype=torch.float64).view(1, 8, 1, 1)
    per = l1 * norm * m * coding / 8.0 * on[:, None].double()
    s += list(per.sum(dim=(0, 2, 3)))
    return dict(x=x, r=r, s=s, sizes=sizes, t=t.detach(), pos=pos, prob=prob.detach(), fg=fg, u=u)


def loss_table(entries: Sequence[Entry], params: Params, aff_maps: Optional[Sequence[torch.Tensor]] = None, grad_scale: float = 1.0,
               device_factor: float = 1.0) -> TableResult:
    """The three kernel families: a table of entries with global normalisers and a totals row (one entry: the one-level entry points'
    row); ``aff_maps``: the ``_aff`` form.  ``device_factor`` is what the caller left in [15] of the totals row before backward."""
    n = len(entries)
    parts = [_entry_forward(e, params, None if aff_maps is None else aff_maps[k]) for k, e in enumerate(entries)]
    smoothing, cls_w = fp32(params.smoothing), fp32(params.cls_weight)
    total_fg = sum(float(q["s"][3]) for q in parts) + smoothing
    total_obj = float(max(sum(int(e.num_objects) for e in entries), 1))
    rows = torch.zeros((n + 1, SUMS_LEN), dtype=torch.float64)
    sizes = torch.full((n + 1, SUMS_LEN), NAN, dtype=torch.float64)
    total = 0.0
    for k, q in enumerate(parts):
        s = q["s"]
        cls = s[0] / total_fg
        coord, dim, rot = (s[4] + s[5] + s[6]) / total_obj, (s[7] + s[8] + s[9]) / total_obj, (s[10] + s[11]) / total_obj
        loss = cls + (coord + dim + rot)
        total = total + loss
        s_, reg = [float(v.detach()) for v in s], [float(v.detach()) for v in (coord, dim, rot, coord + dim + rot)]
        vals = s_ + [total_obj, total_fg, 0.0, 1.0, float(loss.detach()), s_[0] / total_fg, s_[1] / total_fg, s_[2] / total_fg] + reg
        rows[k] = torch.tensor(vals, dtype=torch.float64)
        z = [float(v) for v in q["sizes"]]
        sizes[k, 0], sizes[k, 1], sizes[k, 2] = z[0], z[1], z[2]
        sizes[k, 17], sizes[k, 18], sizes[k, 19] = z[0] / total_fg, z[1] / total_fg, z[2] / total_fg
        sizes[k, 16] = z[0] / total_fg + reg[3]
    rows[n, 16:24] = rows[:n, 16:24].sum(dim=0)
    rows[n, 12], rows[n, 13], rows[n, 15] = n * total_obj, n * total_fg, 1.0
    sizes[n, 16:20] = sizes[:n, 16:20].sum(dim=0)
    scale = fp32(grad_scale) * float(device_factor)
    (total * scale).backward()
    out = []
    for q in parts:
        d_l = q["x"].grad.permute(0, 2, 3, 1).contiguous()
        d_r = q["r"].grad.permute(0, 2, 3, 1).contiguous()
        t, prob = q["t"], q["prob"]
        size_pos = cls_w * abs(scale) / total_fg * t * torch.maximum(prob, t)
        size_dl = torch.where(q["pos"], size_pos, q["x"].grad.abs()).permute(0, 2, 3, 1).contiguous()
        stratum = torch.where(q["pos"], 0, torch.where(q["x"].detach() >= TAIL_X, 1, 2)).permute(0, 2, 3, 1).contiguous()
        out.append(EntryResult(t, q["fg"].double(), d_l, d_r, size_dl, stratum, q["u"]))
    return TableResult(rows, sizes, out)


def loss_one(entry: Entry, params: Params, **kw) -> TableResult:
    """``rv_detection_loss_forward`` / ``_backward``: row 0 of the table of one entry."""
    return loss_table([entry], params, **kw)


TAIL_X = -2.0
D_LOGITS_STRATA = ("d_logits_pos", "d_logits_neg", "d_logits_tail")
MEASURED = ("cls_sums", "cls_scalars", "soft") + D_LOGITS_STRATA


def figures(ref: TableResult, k: int, row=None, soft=None, d_logits=None) -> Dict[str, float]:
    """Worst error of the measured quantities of entry ``k`` in the units of the module docstring.  ``row``: the 24 sums of the entry (or
    a dict {index: value} of some of them), ``soft`` (B,n_cls,H,W), ``d_logits`` (B,H,W,n_cls); whatever is None is left out."""
    out = {}
    er = ref.entries[k] if k < len(ref.entries) else None
    if row is not None:
        items = row.items() if isinstance(row, dict) else enumerate(row.tolist())
        for j, v in items:
            if j in (0, 1, 2, 16, 17, 18, 19):
                key = "cls_sums" if j < 3 else "cls_scalars"
                err = abs(float(v) - float(ref.rows[k, j])) / float(ulp32(ref.sizes[k, j]))
                out[key] = max(out.get(key, 0.0), err if math.isfinite(err) else math.inf)
    if soft is not None:
        err = (soft.double() - er.soft).abs() / ulp32(er.soft)
        out["soft"] = float(torch.nan_to_num(err, nan=math.inf).max())
    if d_logits is not None:
        err = (d_logits.double() - er.d_logits).abs() / ulp32(er.size_d_logits)
        err = torch.nan_to_num(err, nan=math.inf)
        for i, key in enumerate(D_LOGITS_STRATA):
            sel = er.stratum == i
            out[key] = float(err[sel].max()) if bool(sel.any()) else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle_loss(e: Entry, p: Params, dtype):
    """``oracle.targets.detection_loss`` on one entry in ``dtype`` (fp32: the yardstick of the measured comparisons; fp64: the check of
    this file).  Returns (its dict, d_logits (B,H,W,n_cls), d_regressands (B,H,W,8))."""
    from oracle import targets as otgt

    n = e.n_cls
    x = e.logits[..., :n].permute(0, 3, 1, 2).to(dtype).clone().requires_grad_(True)
    r = e.regressands[..., :8].permute(0, 3, 1, 2).to(dtype).clone().requires_grad_(True)
    tg = {"classification_labels": e.labels, "panoptics": e.panoptics[:, None], "regression_targets": e.reg_targets.to(dtype),
          "points_per_obj": e.points_per_obj[:, None]}
    out = otgt.detection_loss(x, r, e.cart.to(dtype), (e.mask != 0)[:, None], tg, n, p.cls_weight, p.reg_weight, list(p.coding_weights),
                              p.smoothing, p.sigma, p.alpha, p.gamma, bool(p.az_inv))
    out["loss"].backward()
    return out, x.grad.permute(0, 2, 3, 1), r.grad.permute(0, 2, 3, 1)


ORACLE_ROW = {16: "loss", 17: "classification_loss", 18: "foreground_loss", 19: "background_loss"}


def oracle_fp32_figures(e: Entry, p: Params, ref: Optional[TableResult] = None) -> Dict[str, float]:
    """The error of the fp32 oracle against this reference on one entry, in the units of ``figures``."""
    ref = ref or loss_one(e, p)
    out, d_l, _ = oracle_loss(e, p, torch.float32)
    assert torch.equal(out["foreground"][:, 0].double(), ref.entries[0].foreground), "the fp32 oracle's foreground differs from the reference's"
    # (smoothing 0: the oracle's regression part is 0 x inf off the instances, and with it its total; the classification scalars stand)
    keys = {j: k for j, k in ORACLE_ROW.items() if j != 16 or fp32(p.smoothing) != 0}
    return figures(ref, 0, row={j: float(out[k].detach()) for j, k in keys.items()}, soft=out["targets"], d_logits=d_l)


# ---------------------------------------------------------------------------------------------------------------- synthetic entries
CODING = (0.5, 1.0, 1.5, 2.0, 0.25, 3.0, 0.75, 1.25)  # eight distinct weights, exact in fp32
DEFAULT = Params()
OPTIONS = {  # every option one at a time, and all together (values exact in fp32)
    "default": DEFAULT,
    "coding": DEFAULT.replace(coding_weights=CODING),
    "cls_weight": DEFAULT.replace(cls_weight=0.5),
    "reg_weight": DEFAULT.replace(reg_weight=2.5),
    "smoothing_half": DEFAULT.replace(smoothing=0.5),
    "smoothing_zero": DEFAULT.replace(smoothing=0.0),
    "sigma_quarter": DEFAULT.replace(sigma=0.25),
    "alpha": DEFAULT.replace(alpha=0.25),
    "gamma_1.5": DEFAULT.replace(gamma=1.5),
    "gamma_1": DEFAULT.replace(gamma=1.0),
    "gamma_0": DEFAULT.replace(gamma=0.0),
    "az_inv_0": DEFAULT.replace(az_inv=False),
    "all": Params(CODING, 0.5, 2.5, 0.5, 0.25, 0.25, 1.5, False),
}


def make_entry(seed: int, B: int, H: int, W: int, n_cls: int, ld_logits: Optional[int] = None, ld_reg: int = 8, instances: int = 3,
               underflow: bool = False, empty: bool = False, mask_zero: bool = False) -> Entry:
    """A synthetic entry from a seeded CPU generator; no target kernel is involved.

    * ``panoptics``: ``instances`` random rectangles per sweep (later ones overwrite earlier ones) plus one at the very end of the last
      row of the last sweep (the pixels a ragged last workgroup / grid-stride pass owns); one label per instance, background label
      ``n_cls``; ``points_per_obj`` = the instance's pixel count; ``num_objects`` = distinct ids per sweep, summed.  ``empty``: none.
    * cart at 5 .. 60 m; mask with about 10 % zeros, one of them forced onto an instance pixel; ``mask_zero``: all zero.
    * targets on instance pixels: offsets in [-0.5, 0.5], log-dimensions in [-1, 1.5], sin / cos in [-1, 1]; 0 elsewhere.
    * regressands = targets + delta on instance pixels (N(0, 1) elsewhere): delta is EXACTLY 0 on a quarter of the elements and on whole
      pixels (8 %; there the affinity is exactly 1 under azimuth-invariant targets), else |delta| in [2^-10, 2^-1]: the sign of
      ``r - t`` is never in doubt.  ``underflow`` (for sigma = 0.25): on 10 % of the instance pixels delta[0] = +-(11 .. 13) m, so that
      d / sigma^2 > 125 and the affinity is 0 in fp32 -- an instance pixel that is not foreground.  Otherwise d < 3.7 m
      (d / sigma^2 < 60 at sigma = 0.25): ``gaussian_affinity`` asserts that nothing falls between.
    * logits N(0, 3) with +-30 and +-90 planted (1 % each, and on 10 % of the instance pixels' own class).
    * padding columns of logits / regressands hold NaN."""
    g = torch.Generator().manual_seed(seed)
    ld_logits = n_cls if ld_logits is None else ld_logits

    def rand(*shape):
        return torch.rand(shape, generator=g, dtype=torch.float64)

    def randint(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    pan = torch.zeros((B, H, W), dtype=torch.int64)
    labels = torch.full((B, H, W), n_cls, dtype=torch.int64)
    ppo = torch.zeros((B, H, W), dtype=torch.int64)
    num_objects = 0
    if not empty:
        for b in range(B):
            for k in range(1, instances + 1):
                h, w = randint(1, max(H // 2, 1)), randint(1, min(max(W // 3, 1), 48))
                y0, x0 = randint(0, H - h), randint(0, W - w)
                pan[b, y0:y0 + h, x0:x0 + w] = k
        pan[B - 1, H - 1, W - min(max(W // 4, 1), 40):] = instances + 1
        for b in range(B):
            ids = pan[b].unique()
            ids = ids[ids > 0]
            num_objects += int(ids.numel())
            for k in ids.tolist():
                sel = pan[b] == k
                labels[b][sel] = randint(0, n_cls - 1)
                ppo[b][sel] = int(sel.sum())
    inst = pan > 0
    flat = inst.flatten().nonzero().flatten()
    rng, az, el = 5.0 + 55.0 * rand(B, H, W), (rand(B, H, W) * 2 - 1) * math.pi, (rand(B, H, W) - 0.5) * 0.5
    cart = torch.stack([rng * el.cos() * az.cos(), rng * el.cos() * az.sin(), rng * el.sin()], dim=1).float()
    mask = (rand(B, H, W) > 0.1)
    if flat.numel() >= 4:
        mask.view(-1)[flat[0]] = False
    if mask_zero:
        mask[:] = False
    tg = torch.cat([rand(B, 3, H, W) - 0.5, rand(B, 3, H, W) * 2.5 - 1.0, rand(B, 2, H, W) * 2 - 1], dim=1).float() * inst[:, None]
    delta = torch.exp2(-10.0 + 9.0 * rand(B, 8, H, W)) * (torch.randint(0, 2, (B, 8, H, W), generator=g) * 2 - 1)
    delta = delta * (rand(B, 8, H, W) >= 0.25)
    exact = inst & (rand(B, H, W) < 0.08)
    if flat.numel() >= 2:
        exact.view(-1)[flat[1]] = True
    delta = delta * (~exact)[:, None]
    far = torch.zeros_like(inst)
    if underflow:
        far = inst & ~exact & (rand(B, H, W) < 0.1)
        if flat.numel() >= 3:
            far.view(-1)[flat[2]] = True
            exact.view(-1)[flat[2]] = False
        delta[:, 0] = torch.where(far, (11.0 + 2.0 * rand(B, H, W)) * (torch.randint(0, 2, (B, H, W), generator=g) * 2 - 1), delta[:, 0])
    noise = torch.randn((B, 8, H, W), generator=g, dtype=torch.float64).float()
    reg = torch.where(inst[:, None], tg + delta.float(), noise)
    diff = reg - tg
    on = inst[:, None].expand_as(diff)
    assert bool(((diff == 0) == (delta == 0))[on].all()) and bool((diff.abs() >= 2.0 ** -11)[on & (delta != 0)].all())
    x = torch.randn((B, n_cls, H, W), generator=g, dtype=torch.float64) * 3.0
    planted = torch.zeros((B, n_cls, H, W), dtype=torch.bool)
    for v in (30.0, -30.0, 90.0, -90.0):
        sel = rand(B, n_cls, H, W) < 0.01
        x[sel] = v
        planted |= sel
    own = (labels[:, None] == torch.arange(n_cls).view(1, n_cls, 1, 1)) & (rand(B, 1, H, W) < 0.1)
    x[own] = torch.tensor([30.0, -30.0, 90.0, -90.0], dtype=torch.float64)[torch.randint(0, 4, (int(own.sum()),), generator=g)]
    planted |= own
    logits = torch.full((B, H, W, ld_logits), NAN, dtype=torch.float32)
    logits[..., :n_cls] = x.float().permute(0, 2, 3, 1)
    regressands = torch.full((B, H, W, ld_reg), NAN, dtype=torch.float32)
    regressands[..., :8] = reg.permute(0, 2, 3, 1)
    return Entry(logits, regressands, cart.contiguous(), mask.to(torch.uint8), labels, pan, tg.contiguous(), ppo, num_objects, n_cls,
                 {"exact": exact, "far": far, "logits": planted})


def make_affinity_map(e: Entry, seed: int) -> torch.Tensor:
    """An affinity map as ``rv_soft_assign`` leaves one: 0 off the instances, on them values in (0.05, 1) with a fifth exactly 0 (top-k
    dropouts) and a tenth exactly 1."""
    g = torch.Generator().manual_seed(seed)
    B, H, W = e.shape
    a = 0.05 + 0.95 * torch.rand((B, H, W), generator=g)
    pick = torch.rand((B, H, W), generator=g)
    a = torch.where(pick < 0.2, torch.zeros_like(a), a)
    a = torch.where(pick > 0.9, torch.ones_like(a), a)
    inst = e.panoptics > 0
    flat = inst.flatten().nonzero().flatten()
    if flat.numel() >= 3:
        a.view(-1)[flat[0]], a.view(-1)[flat[1]], a.view(-1)[flat[2]] = 0.0, 1.0, 0.625
    return (a * inst).float().contiguous()


# The entries the fp32 oracle is measured on (tests/test_loss_ref_cpu.py prints the figures; tests/test_gpu_loss_kernels.py derives the
# kernel's bounds from them): every option setting on the ragged one-entry shape, with the class counts of both row forms.
def yardstick_cases():
    cases = []
    for i, (name, p) in enumerate(OPTIONS.items()):
        for n_cls, ld in ((3, 32), (26, 32), (7, 40)):
            cases.append((f"{name}-{n_cls}", make_entry(1000 + 7 * i + n_cls, 2, 5, 67, n_cls, ld, 8, underflow=fp32(p.sigma) == 0.25), p))
    return cases


_YARDSTICK: Dict[str, float] = {}


def oracle_yardstick() -> Dict[str, float]:
    """Worst figure of the fp32 oracle per measured quantity over ``yardstick_cases`` (computed once per process).  The oracle reports
    no un-normalised sums: ``cls_sums`` takes the figure of the scalars, which are the same numbers over total_fg."""
    if not _YARDSTICK:
        worst: Dict[str, float] = {}
        for _, e, p in yardstick_cases():
            for k, v in oracle_fp32_figures(e, p).items():
                worst[k] = max(worst.get(k, 0.0), v)
        worst["cls_sums"] = worst["cls_scalars"]
        _YARDSTICK.update(worst)
    return dict(_YARDSTICK)


# Negatives with x < TAIL_X, where the fp32 oracle is no yardstick (tests/test_loss_ref_cpu.py, FINDING): a bound from the precision of the
# formats, for ANY fp32 evaluation of alpha * p^gamma * (gamma (1 - p) softplus(x) + p) * cls_weight * mask / total_fg from e = exp(x),
# p = e / (1 + e), softplus = log1p(e), with 0 <= gamma <= 2 and library functions good to 2 ulp (exp, log1p) and 4 ulp (pow).  In
# units of 2^-24 relative: e 2, p 3 (one addition that barely moves, one division), softplus 4, p^gamma <= 2 x 3 + 4 = 10, 1 - p 1
# (p < 0.12), gamma (1 - p) softplus 6, the bracket (two positive terms) 6.5, the product of the three 18, the weight, the fp64
# normaliser and the rounding to fp32 19; an error of 2^-24 relative is at most 2 ulp at the bottom of a binade: 38, rounded up.
# The 2 ulp of exp / log1p and the 4 ulp of pow are ASSUMED of the device's library (the figures its documentation gives for these
# functions); nobody has measured them on the device.  A library worse than that would show here as a failure, not be absorbed.
TAIL_ULP = 40.0


def kernel_bounds(same_inputs: Optional[Dict[str, float]] = None) -> Dict[str, float]:
    """Twice the fp32 oracle's worst figure and no less than 4 ulp: the device's expf / log1pf / sin / cos are allowed a couple of ulp
    the host libm does not spend.  The worst figure is taken over ``yardstick_cases`` and, where given, the oracle's figures on the SAME
    inputs as the kernel's (``oracle_fp32_figures``: a case of half a million pixels has rarer elements than the yardstick's 670).
    The tail stratum of ``d_logits`` takes ``TAIL_ULP`` where that is the smaller number."""
    y = oracle_yardstick()
    if same_inputs:
        y = {k: max(v, same_inputs.get(k, 0.0), same_inputs.get("cls_scalars", 0.0) if k == "cls_sums" else 0.0) for k, v in y.items()}
    b = {k: max(4.0, 2.0 * v) for k, v in y.items()}
    b["d_logits_tail"] = min(b["d_logits_tail"], TAIL_ULP)
    return b
