"""``loss_ref.py`` (the fp64 restatement of the fused detection loss that tests/test_gpu_loss_kernels.py holds the kernels to) is itself
checked here, on the CPU:

* against the reference's own numbers: the ``tiny_model`` fixture (loss dict, soft targets, foreground; it stores no gradient of the
  head outputs) and every ``multilevel/*`` fixture (loss dict, soft targets, foreground, ``d_logits``, ``d_regressands``), at the bounds
  the fixtures' own tests use (test_oracle_golden.py, test_multilevel_golden.py, test_gpu_multilevel.py);
* against ``oracle.targets.detection_loss`` run in fp64 on synthetic entries with every non-default option.  The two differ where the
  operation is DEFINED in fp32 and the fp64 oracle is not: the decoded centres (rounded to fp32: at most sqrt(3) ulp(73 m) = sqrt(3) 2^-17
  in the distance, so a relative ``TOL_T = sqrt(3) 2^-17 / sigma^2`` in the affinity) and ``|r - t| * reg_weight`` (two fp32 roundings:
  2^-23 relative).  Everything downstream is bounded by propagating these two, element by element, to first order;
* the error of the same oracle run in fp32, in the units of ``loss_ref.figures``: the yardstick of the measured comparisons of
  tests/test_gpu_loss_kernels.py.  Printed (``pytest -s``); figures of one x86-64 host are in that module's docstring.

FINDING (the fp32 oracle, not the kernels): on NEGATIVE elements torch forms BCE-with-logits as ``(1 - t) x - log_sigmoid(x)``; at
x < 0 that is ``x - (x - log1p(e^x))`` in fp32 and loses log2(|x| / e^x) bits -- 1e-3 relative at x = -8.7, a factor 3 at x = -30.  The
figure of ``d_logits`` is therefore taken per stratum (positives; negatives with x >= -2; negatives with x < -2, ``d_logits_tail``), and in
the last stratum the oracle is no yardstick (1e7 ulp).
"""

from __future__ import annotations

import math

import pytest
import torch

import loss_ref as R
from test_multilevel_golden import CASES, LOSS_KEYS, case_entries
from test_oracle_golden import close, unpack

INDEX = {"loss": 16, "classification_loss": 17, "foreground_loss": 18, "background_loss": 19, "regression_loss": 23, "coordinate_loss": 20,
         "dimension_loss": 21, "rotation_loss": 22, "total_fg": 13, "total_objects": 12}


def fixture_entry(logits, regressands, cart, mask, tg, n_cls):
    """An ``Entry`` (NHWC, no padding) from the NCHW tensors of a fixture."""
    pan = tg["panoptics"].reshape(mask.shape[0], *mask.shape[-2:])
    n_obj = sum(int((x.unique() > 0).sum()) for x in pan)
    return R.Entry(logits.permute(0, 2, 3, 1).contiguous(), regressands.permute(0, 2, 3, 1).contiguous(), cart.contiguous(),
                   mask.reshape(pan.shape).to(torch.uint8), tg["classification_labels"], pan, tg["regression_targets"].contiguous(),
                   tg["points_per_obj"].reshape(pan.shape), n_obj, n_cls)


def test_reference_reproduces_the_tiny_model_fixture(golden):
    g = golden("tiny_model")
    tg = {k: g[f"targets/{k}"] for k in ("classification_labels", "panoptics", "regression_targets", "points_per_obj")}
    e = fixture_entry(g["logits"], g["regressands"], g["cart"], g["mask"], tg, 5)
    ref = R.loss_one(e, R.DEFAULT)
    close(ref.entries[0].soft, g["targets/soft"], 1e-5, "soft targets")
    assert torch.equal(ref.entries[0].foreground.float(), g["aux/foreground"][:, 0])
    for k, j in INDEX.items():
        close(ref.rows[0, j].reshape(()), g[f"loss/{k}"].reshape(()), 5e-5, f"loss {k}")
    assert int(ref.rows[0, 3]) == int(g["aux/foreground"].sum()) > 20 and float(ref.rows[0, 15]) == 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_reference_reproduces_the_multilevel_fixtures(golden, name):
    g0, g, case = golden("multilevel/common"), golden(f"multilevel/{name}"), CASES[name]
    fix = case_entries(g0, g, name)
    entries = [fixture_entry(f["logits"], f["regressands"], f["cart"], f["mask"], f["targets"], f["n_cls"]) for f in fix]
    ref = R.loss_table(entries, R.DEFAULT)
    n = len(entries)
    want = unpack(g, "loss")
    got = {k: float(ref.rows[n, j]) for k, j in INDEX.items()}
    for i, s in enumerate(case["strides"]):  # (``/s{stride}`` is entry i of the reference's collated list for the i-th stride)
        got.update({f"{k}/s{s}": float(ref.rows[i, j]) for k, j in INDEX.items()})
    assert set(got) == set(want) and set(LOSS_KEYS) == set(INDEX)
    for k, v in want.items():
        assert abs(got[k] - float(v)) <= 1e-6 * max(1.0, abs(float(v))), (name, k, got[k], float(v))
    for f, er in zip(fix, ref.entries):
        p = f["prefix"]
        assert torch.allclose(er.soft.float(), g[f"{p}/soft"], atol=1e-6), (name, p)
        assert torch.equal(er.foreground.float(), g[f"{p}/foreground"][:, 0]), (name, p)
        for key, mine in (("d_logits", er.d_logits), ("d_regressands", er.d_regressands)):
            w = g[f"{p}/{key}"].permute(0, 2, 3, 1).double()
            assert float((mine - w).abs().max()) <= 1e-5 * float(w.abs().max()), (name, p, key)


SYNTHETIC = [(name, n_cls, ld) for name in R.OPTIONS if name != "default" for n_cls, ld in ((3, 32), (7, 40))]


@pytest.mark.parametrize("name,n_cls,ld", SYNTHETIC, ids=[f"{a}-{b}" for a, b, _ in SYNTHETIC])
def test_reference_agrees_with_the_fp64_oracle(name, n_cls, ld):
    """No underflow pixels here: in fp64 ``exp(-139)`` is not 0, and whether such a pixel is foreground is the fp32 definition."""
    p = R.OPTIONS[name]
    e = R.make_entry(77 + n_cls, 2, 5, 67, n_cls, ld, 12)
    ref = R.loss_one(e, p)
    out, d_l, d_r = R.oracle_loss(e, p, torch.float64)
    er, row = ref.entries[0], ref.rows[0]
    assert torch.equal(out["foreground"][:, 0], er.foreground) and float(out["total_fg"]) == float(row[13]) and float(out["total_objects"]) == float(row[12])
    assert int(row[3]) > 20 and bool(e.planted["exact"].any())
    tol_t = math.sqrt(3.0) * 2.0 ** -17 / R.fp32(p.sigma) ** 2
    t = er.soft
    assert bool(((out["targets"] - t).abs() <= tol_t * t).all())
    assert bool((t.permute(0, 2, 3, 1)[e.planted["exact"] & (e.panoptics > 0)].sum(-1) == 1.0).all()) or not p.az_inv
    # classification: d(t (softplus(x) - x t)) = dt (softplus(x) - 2 x t); d(t (p - t)) = dt (p - 2 t); negatives carry no t, but the
    # oracle's own bce cancels there (module docstring) by up to ulp64(|x|) = 2^-46 at |x| <= 90, absolutely
    x = e.logits[..., :n_cls].permute(0, 3, 1, 2).double()
    sp, prob, m = R._softplus(x), torch.sigmoid(x), (e.mask != 0).double()[:, None]
    cls_w, total_fg = R.fp32(p.cls_weight), float(row[13])
    bce_abs = R.fp32(p.alpha) * 2.0 ** -46
    el = cls_w * m * (tol_t * t * (sp + 2 * x.abs() * t) + (t == 0) * bce_abs) / total_fg
    fg, bg = er.foreground[:, None], (1 - er.foreground[:, None]) * m
    for key, j, w in (("classification_loss", 17, 1.0), ("foreground_loss", 18, fg), ("background_loss", 19, bg)):
        assert abs(float(out[key]) - float(row[j])) <= float((el * w).sum()) + 1e-12 * abs(float(row[j])), (key, float(out[key]), float(row[j]))
    el_g = (cls_w * m * (tol_t * t * (prob + 2 * t) + (t == 0) * bce_abs * 3) / total_fg).permute(0, 2, 3, 1)
    assert bool(((d_l - er.d_logits).abs() <= el_g + 1e-9 * er.d_logits.abs()).all())
    # regression: 2^-23 relative on every term of the sums (all of one sign); the gradient has no fp32 step
    if R.fp32(p.smoothing) != 0:  # (smoothing 0: the oracle's regression part is 0 x inf off the instances)
        for key, j in (("coordinate_loss", 20), ("dimension_loss", 21), ("rotation_loss", 22), ("regression_loss", 23)):
            assert abs(float(out[key]) - float(row[j])) <= 2.0 ** -22 * float(row[j]), key
        assert abs(float(out["loss"]) - float(row[16])) <= float(el.sum()) + 2.0 ** -22 * float(row[16])
        assert bool(((d_r - er.d_regressands).abs() <= 1e-12 * er.d_regressands.abs()).all())
    assert bool((er.d_regressands[e.labels == n_cls] == 0).all()) and bool((er.d_regressands[e.mask == 0] == 0).all())


def test_fp32_oracle_yardstick(capsys):
    """The figures the kernel's bounds are made of: the worst error of the fp32 oracle per measured quantity over every option setting,
    class counts of both row forms.  Also what the synthetic entries are for: every case has foreground, an affinity of exactly 1 and,
    at sigma 0.25, instance pixels whose affinity underflows."""
    worst = {}
    for name, e, p in R.yardstick_cases():
        ref = R.loss_one(e, p)
        er = ref.entries[0]
        inst = e.panoptics > 0
        assert int(ref.rows[0, 3]) > 20 and e.num_objects >= 3
        if p.az_inv:
            assert bool((er.soft.sum(1)[e.planted["exact"]] == 1.0).all()) and bool(e.planted["exact"].any())
        if R.fp32(p.sigma) == 0.25:
            far = e.planted["far"]
            assert int(far.sum()) >= 3 and bool((er.foreground[far] == 0).all()) and bool((er.affinity_arg[far] > 125).all())
        assert bool((er.affinity_arg[inst & ~e.planted["far"]] < 60).all())
        f = R.oracle_fp32_figures(e, p, ref)
        assert all(math.isfinite(v) for v in f.values()), (name, f)
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
    with capsys.disabled():
        print("\nfp32 oracle vs loss_ref, worst fp32 ulps: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    y, b = R.oracle_yardstick(), R.kernel_bounds()
    assert all(y[k] == worst[k] for k in worst) and y["cls_sums"] == y["cls_scalars"]
    assert set(b) == set(R.MEASURED) and all(v >= 4.0 for v in b.values())
    # the finding of the module docstring: only the tail stratum is beyond a few dozen ulp
    assert all(y[k] < 100 for k in y if k != "d_logits_tail") and y["d_logits_tail"] > 1e4
