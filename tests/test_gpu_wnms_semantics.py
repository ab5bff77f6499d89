"""The weighted-NMS choices (``RV_WNMS_*`` / ``WnmsSemantics``) on the device: the list entry (``rv_wnms_opt``) and the batch entry
(``rv_nms_sweeps_opt``) against the numpy restatement of all 16 settings (``tests/wnms_semantics_ref.py``), the per-class fallback loop,
the defaults against the existing entries, ``RangeDecoder.decode``, the TorchEx-shaped shim and the pin tool.

Bar: list entry -- ``keep``, ``count`` and ``output`` bit-equal (same fp32 inputs, same unfused arithmetic, same summation order).  Batch
entry -- rows, order, classes and sweep index exact, x y z l w h and the score bit-equal; the yaw is ``atan2`` of merged ``sin`` / ``cos``
columns that the two sides compute with different libraries (device ``sinf`` / ``atan2f`` against torch's on the CPU): 1e-6 of the
maximum, the tolerance of ``tests/test_gpu_nms_wrapper.py``.  The lists are axis-aligned with dyadic coordinates, so an IoU can equal a
threshold bit for bit (checked on the CPU in ``tests/test_wnms_semantics_cpu.py``).
"""

from __future__ import annotations

import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import wnms_semantics_ref as ref
from test_gpu_forward import DEV, rel_err

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import pin_wnms  # noqa: E402

sys.path.pop(0)

pytestmark = pytest.mark.gpu

SETTINGS = ref.ALL_SETTINGS


def _hnms():
    from range_view_3d_detection_amd.math.ops import nms as hnms

    return hnms


def _device_list(boxes, data, nms_t, merge_t, semantics, cats=None):
    """``rv_wnms_opt`` (``rv_wnms`` for semantics None without classes) on one sorted list -> numpy (keep, output, count)."""
    hnms = _hnms()
    b, d = torch.from_numpy(boxes).to(DEV), torch.from_numpy(data).to(DEV)
    c = None if cats is None else torch.from_numpy(cats).to(DEV)
    n = d.shape[0]
    out = torch.zeros_like(d)
    keep = torch.zeros(n, dtype=torch.long, device=DEV)
    count = torch.zeros(n, dtype=torch.long, device=DEV)
    k = hnms.wnms_sorted(b, d, out, keep, count, nms_t, merge_t, semantics, cats=c)
    assert not out[k:].any()  # the reference wrapper's post-condition (nms.py:173)
    return keep[:k].cpu().numpy(), out[:k].cpu().numpy(), count[:k].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(boxes, data, cats or None, nms_thresh, merge_thresh) of a named list."""
    if name[1:].isdigit():
        b, d, _ = ref.random_list(int(name[1:]), 100 + int(name[1:]))
        return b, d, None, 0.3, 0.5
    if name in ("classes", "no_classes"):
        b, d, c = ref.random_list(200, 7)
        return b, d, (c if name == "classes" else None), 0.3, 0.5
    if name == "chain":
        return (*ref.chain_list(), None, 0.3, 0.5)
    if name == "thresholds":
        return (*ref.threshold_list(), None, 0.3, 0.5)
    if name == "equal_thresholds":
        return (*ref.threshold_list(), None, 0.5, 0.5)
    if name == "scores":
        return (*ref.score_list(), None, 0.3, 0.5)
    if name == "zero_thresholds":
        return (*ref.far_list(), None, 0.0, 0.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want_list(name, flags):
    b, d, c, nms_t, merge_t = _case(name)
    return ref.wnms_sorted(b, d, nms_t, merge_t, ref.WnmsSemantics.from_flags(flags), c)


@pytest.mark.parametrize("name", ["n1", "n63", "n64", "n65", "n130", "classes", "no_classes", "chain", "thresholds", "equal_thresholds",
                                  "scores", "zero_thresholds"])
def test_list_entry_equals_the_restatement_under_all_sixteen_settings(name):
    b, d, c, nms_t, merge_t = _case(name)
    for s in SETTINGS:
        keep, out, count = _device_list(b, d, nms_t, merge_t, s, c)
        wk, wo, wc = _want_list(name, s.flags)
        assert np.array_equal(keep, wk), (name, s)
        assert np.array_equal(count, wc), (name, s)
        assert out.tobytes() == wo.tobytes(), (name, s)


def test_list_entry_cases_by_their_own_properties():
    """What each hand-built list is for, stated on the device results themselves."""
    for s in SETTINGS:
        # chain A (3), C (70), B (130) across three mask words: A suppresses and merges B; C takes the suppressed B under ALL only
        keep, out, count = _device_list(*ref.chain_list(), 0.3, 0.5, s)
        at = dict(zip(keep.tolist(), count.tolist()))
        assert 130 not in at and at[3] == 2 and at[70] == (2 if s.merge_set == "ALL" else 1) and len(at) == 139, s
        # pairs AT the thresholds: (0,1) at fp32(0.3), (2,3) at 0.5
        b, d = ref.threshold_list()
        keep, out, count = _device_list(b, d, 0.3, 0.5, s)
        at = dict(zip(keep.tolist(), count.tolist()))
        assert (1 in at) == (s.nms_compare == "GT") and at[0] == 1 and 3 not in at and at[2] == (2 if s.merge_compare == "GE" else 1), s
        keep, out, count = _device_list(b, d, 0.5, 0.5, s)  # one pair at both thresholds
        at = dict(zip(keep.tolist(), count.tolist()))
        assert (3 in at) == (s.nms_compare == "GT") and at[2] == (2 if s.merge_compare == "GE" else 1), s
        # score column: the keeper's own score, bitwise; the other columns do not move
        b, d = ref.score_list()
        keep, out, count = _device_list(b, d, 0.3, 0.5, s)
        mean = _device_list(b, d, 0.3, 0.5, ref.WnmsSemantics(s.merge_set, "MEAN", s.nms_compare, s.merge_compare))[1]
        assert keep.tolist() == [0, 1] and count.tolist() == [3, 3] and out[:, :-1].tobytes() == mean[:, :-1].tobytes(), s
        assert (out[:, -1].tobytes() == d[[0, 1], -1].tobytes()) == (s.score == "KEEPER"), s
        # thresholds of 0 on far-apart boxes (every IoU is 0): `0 >= 0` passes for every pair -- no far-pair skip in such a call
        b, d = ref.far_list()
        n = b.shape[0]
        keep, out, count = _device_list(b, d, 0.0, 0.0, s)
        if s.nms_compare == "GE":
            assert keep.tolist() == [0] and count.tolist() == [n if s.merge_compare == "GE" else 1], s
        else:
            assert keep.tolist() == list(range(n)) and count.tolist() == ([n - i for i in range(n)] if s.merge_compare == "GE" else [1] * n), s


# ------------------------------------------------------------------------------------------------------------------------------------
# batch entry
# ------------------------------------------------------------------------------------------------------------------------------------
PRE, POST = 100, 40  # class 0 holds ~150 of a sweep's 300 candidates: cut by num_pre_nms; classes 1 and 2 keep > 40 rows: cut by num_post_nms


@functools.lru_cache(maxsize=None)
def _sweeps():
    return ref.sweeps()


@functools.lru_cache(maxsize=None)
def _want_batch(flags):
    cub, sc, ct = _sweeps()
    return ref.batched_multiclass_nms(cub, sc, ct, PRE, POST, 0.3, 0.1, ref.WnmsSemantics.from_flags(flags))


def _device_batch(semantics, cub=None, sc=None, ct=None, pre=PRE, post=POST, thr=0.3, conf=0.1, n_classes=3, **kw):
    if cub is None:
        cub, sc, ct = _sweeps()
    return _hnms().batched_multiclass_nms(cub.to(DEV), sc.to(DEV), ct.to(DEV), pre, post, thr, conf, "WEIGHTED", n_classes=n_classes,
                                          semantics=semantics, **kw)


def _same_batch(got, want, what):
    p, s, c, b = (t.cpu() for t in got)
    wp, ws, wc, wb = want
    assert len(set(zip(ws.tolist(), wc.tolist(), wb.tolist()))) == len(ws), "equal scores in a class: topk leaves their order open"
    assert p.shape == wp.shape and s.shape == ws.shape, (what, tuple(p.shape), tuple(wp.shape))
    assert torch.equal(c, wc) and torch.equal(b, wb), f"{what}: classes / sweeps / row order differ"
    assert torch.equal(s, ws), f"{what}: scores differ"
    assert torch.equal(p[:, :6], wp[:, :6]), f"{what}: boxes differ"
    assert rel_err(p[:, 6], wp[:, 6]) < 1e-6, (what, rel_err(p[:, 6], wp[:, 6]))


@pytest.mark.parametrize("flags", range(16))
def test_batch_entry_equals_the_restatement_in_the_per_class_loop(flags):
    s = ref.WnmsSemantics.from_flags(flags)
    want = _want_batch(flags)
    cub, sc, ct = _sweeps()
    for b in range(2):  # class 0 of either sweep holds more than num_pre_nms candidates after the confidence filter: the pre-NMS cut acts
        assert int(((sc[b] >= 0.1) & (ct[b] == 0)).sum()) > PRE
        assert all(0 < int(((sc[b] >= 0.1) & (ct[b] == c)).sum()) <= PRE for c in (1, 2))
    counts = torch.bincount((want[2] + 3 * want[3]).long(), minlength=6)
    assert counts.tolist() == [POST] * 6  # every class of both sweeps is cut by num_post_nms
    _same_batch(_device_batch(s), want, str(s))


def test_batch_settings_do_change_the_rows():
    """The 16 expected results are 16 different results: every axis moves some row of this batch (the clusters for the merge set and
    the score column, the implanted pairs at the thresholds for the two comparisons)."""
    rows = [_want_batch(f) for f in range(16)]
    for i in range(16):
        for j in range(i):
            assert not all(torch.equal(x, y) for x, y in zip(rows[i], rows[j])), (i, j)


def test_batch_resume_under_a_setting():
    """A mask budget below the need: the first ``rv_nms_sweeps_opt`` call reports the words, the resumed one finishes -- same rows."""
    hnms = _hnms()
    s = ref.WnmsSemantics.from_flags(9)
    calls = []
    orig_call = hnms.L.call

    def spy(name, *a):
        calls.append((name, a[-3] if name == "rv_nms_sweeps_opt" else None))  # (`resume` sits before stream and flags)
        return orig_call(name, *a)

    old, hnms.MASK_WORDS = hnms.MASK_WORDS, 40
    hnms.L.call = spy
    try:
        small = _device_batch(s)
    finally:
        hnms.MASK_WORDS, hnms.L.call = old, orig_call
    assert [c for c in calls if c[0].startswith("rv_nms_sweeps")] == [("rv_nms_sweeps_opt", 0), ("rv_nms_sweeps_opt", 1)]
    _same_batch(small, _want_batch(9), "resumed")


@pytest.mark.parametrize("flags", [1, 6, 15])
def test_fallback_loop_equals_the_fused_path(flags):
    hnms = _hnms()
    s = ref.WnmsSemantics.from_flags(flags)
    fused = _device_batch(s)
    old, hnms.FUSED_CLASSES_MAX = hnms.FUSED_CLASSES_MAX, 0
    try:
        loop = _device_batch(s)
    finally:
        hnms.FUSED_CLASSES_MAX = old
    _same_batch(loop, _want_batch(flags), f"loop {s}")
    _same_batch(loop, tuple(t.cpu() for t in fused), f"loop against fused {s}")


def _cuboids_of(data, cats=None):
    """Rows [x,y,z,l,w,h,sin,cos,score] of an axis-aligned list -> one sweep (1,n,7), (1,n), (1,n)."""
    d = torch.from_numpy(data)
    cub = torch.cat([d[:, :6], torch.zeros(d.shape[0], 1)], dim=1)
    ct = torch.zeros(d.shape[0], dtype=torch.long) if cats is None else torch.from_numpy(cats).long()
    return cub[None], d[None, :, 8], ct[None]


def test_batch_top_k_ranks_by_the_score_column():
    """Two clusters of one class, ``num_post_nms`` = 1: by merged score cluster Q (0.79) is ahead, by keeper score cluster P (0.9)."""
    b, d = ref.score_list()
    cub, sc, ct = _cuboids_of(d)
    rows = {}
    for score in ("MEAN", "KEEPER"):
        s = ref.WnmsSemantics(score=score)
        p, sco, c, bi = _device_batch(s, cub, sc, ct, pre=100, post=1, conf=0.05, n_classes=1)
        want = ref.batched_multiclass_nms(cub, sc, ct, 100, 1, 0.3, 0.05, s)
        assert torch.equal(p.cpu()[:, :6], want[0][:, :6]) and torch.equal(sco.cpu(), want[1]) and p.shape[0] == 1
        rows[score] = (float(p[0, 1]), sco.cpu())
    assert abs(rows["MEAN"][0] - 30.5) < 1e-3 and abs(rows["KEEPER"][0] - 0.5) < 1e-3  # y centre of cluster Q / of cluster P
    assert rows["KEEPER"][1].numpy().tobytes() == d[0:1, 8].tobytes()


def test_batch_threshold_zero():
    """Far-apart boxes, ``nms_threshold`` 0: ``GE`` leaves one row per class (no far-pair skip), ``GT`` keeps every box."""
    b, d = ref.far_list()
    cats = (np.arange(b.shape[0]) % 2).astype(np.int32)
    cub, sc, ct = _cuboids_of(d, cats)
    for s in (ref.WnmsSemantics(nms_compare="GE"), ref.WnmsSemantics()):
        p, sco, c, bi = _device_batch(s, cub, sc, ct, pre=100, post=100, thr=0.0, conf=0.0, n_classes=2)
        want = ref.batched_multiclass_nms(cub, sc, ct, 100, 100, 0.0, 0.0, s)
        assert p.shape[0] == (2 if s.nms_compare == "GE" else b.shape[0])
        assert torch.equal(p.cpu()[:, :6], want[0][:, :6]) and torch.equal(sco.cpu(), want[1]) and torch.equal(c.cpu(), want[2])


# ------------------------------------------------------------------------------------------------------------------------------------
# defaults, decoder, shim, errors
# ------------------------------------------------------------------------------------------------------------------------------------
def test_defaults_three_ways():
    """``rv_wnms_opt(flags = 0)`` / ``rv_nms_sweeps_opt(flags = 0)``, the existing entries and ``semantics=None``: bit-equal."""
    hnms = _hnms()
    L = hnms.L
    b, d, c = ref.random_list(200, 7)
    bt, dt, ct = torch.from_numpy(b).to(DEV), torch.from_numpy(d).to(DEV), torch.from_numpy(c).to(DEV)
    n = dt.shape[0]
    ws = torch.empty(L.load().rv_wnms_workspace_bytes(n), dtype=torch.uint8, device=DEV)

    def raw(entry, cats, *tail):
        out, keep, count = torch.zeros_like(dt), torch.zeros(n, dtype=torch.long, device=DEV), torch.zeros(n, dtype=torch.long, device=DEV)
        num = L.i64(0)
        head = (L.ptr(bt), L.ptr(dt)) + (() if entry == "rv_wnms" else (L.ptr(cats),))
        L.call(entry, *head, n, 9, 0.3, 0.5, L.ptr(out), L.ptr(keep), L.ptr(count), L.ptr(ws), ctypes.byref(num), L.stream_ptr(), *tail)
        k = int(num.value)
        return keep[:k].cpu(), out[:k].cpu(), count[:k].cpu()

    for cats in (ct, None):
        results = [raw("rv_wnms_opt", cats, 0), raw("rv_wnms_classes", cats)]
        results.append(tuple(torch.from_numpy(x) for x in _device_list(b, d, 0.3, 0.5, None, None if cats is None else c)))
        results.append(tuple(torch.from_numpy(x) for x in _device_list(b, d, 0.3, 0.5, ref.WnmsSemantics(), None if cats is None else c)))
        if cats is None:
            results.append(raw("rv_wnms", None))
        for r in results[1:]:
            assert all(torch.equal(x, y) for x, y in zip(r, results[0]))
        assert len(results[0][0]) < n and int(results[0][2].max()) >= 2  # (the list does suppress and merge)

    # batch: semantics=None (rv_nms_sweeps), the default setting, and the same call sent to rv_nms_sweeps_opt with flags = 0
    none = _device_batch(None)
    default = _device_batch(ref.WnmsSemantics())
    orig_call, sent = L.call, []

    def to_opt(name, *a):
        if name == "rv_nms_sweeps":
            sent.append(name)
            return orig_call("rv_nms_sweeps_opt", *a, 0)
        return orig_call(name, *a)

    hnms.L.call = to_opt
    try:
        opt0 = _device_batch(None)
    finally:
        hnms.L.call = orig_call
    assert sent == ["rv_nms_sweeps"]
    for r in (default, opt0):
        assert all(torch.equal(x, y) for x, y in zip(r, none))
    _same_batch(none, _want_batch(0), "semantics=None")


def test_range_decoder_reads_wnms_semantics(golden):
    """``post_processing_config["wnms_semantics"]``: absent = today's rows; a plain dict (and an OmegaConf mapping, where that imports)
    reaches the NMS as a ``WnmsSemantics``; under ``score: KEEPER`` every output score is a candidate's score, bit for bit."""
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

    hnms = _hnms()
    t = golden("tiny_model")
    logits, reg = t["eval/logits"], t["eval/regressands"]
    mo = {1: {"cart": t["cart"].to(DEV), "mask": t["mask"].to(DEV), 0: {"logits": logits.to(DEV), "regressands": reg.to(DEV)}}}
    dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    post = {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "WEIGHTED"}
    tasks = {0: ["c"] * logits.shape[1]}
    seen = []
    orig = hnms.batched_multiclass_nms

    def spy(*a, **kw):
        seen.append(kw.get("semantics"))
        return orig(*a, **kw)

    hnms.batched_multiclass_nms = spy
    try:
        absent = dec.decode(mo, post, tasks, use_nms=True)
        default = dec.decode(mo, {**post, "wnms_semantics": {}}, tasks, use_nms=True)
        block = {"merge_set": "ALL", "score": "KEEPER"}
        plain = dec.decode(mo, {**post, "wnms_semantics": block}, tasks, use_nms=True)
        try:
            from omegaconf import OmegaConf
        except ImportError:
            OmegaConf = None
        if OmegaConf is not None:
            oc = dec.decode(mo, OmegaConf.create({**post, "wnms_semantics": block}), tasks, use_nms=True)
            assert all(torch.equal(x, y) for x, y in zip(oc, plain))
    finally:
        hnms.batched_multiclass_nms = orig
    want = ref.WnmsSemantics(merge_set="ALL", score="KEEPER")
    assert seen[:3] == [None, ref.WnmsSemantics(), want] and all(s == want for s in seen[3:])
    assert all(torch.equal(x, y) for x, y in zip(absent, default))
    assert absent[0].shape[0] > 50 and plain[0].shape == absent[0].shape and not torch.equal(plain[1], absent[1])
    candidates = dec.decode(mo, {**post, "min_confidence": 0.0}, tasks, use_nms=False)[1]
    assert bool(torch.isin(plain[1], candidates).all()) and not bool(torch.isin(absent[1], candidates).all())
    with pytest.raises(hnms.L.RvError, match="scoer"):
        dec.decode(mo, {**post, "wnms_semantics": {"scoer": "KEEPER"}}, tasks, use_nms=True)


def _shim():
    from range_view_3d_detection_amd import compat

    sys.path.insert(0, list(compat.__path__)[0])
    try:
        import weighted_nms_ext
    finally:
        sys.path.pop(0)
    return weighted_nms_ext


@pytest.mark.parametrize("flags", range(16))
def test_shim_semantics_block_and_the_pin_tool(flags):
    ext = _shim()
    s = ref.WnmsSemantics.from_flags(flags)
    b, d, _ = ref.random_list(200, 7)
    with ext.semantics(s):
        keep, out, count = pin_wnms.run(ext.wnms_gpu, DEV, b, d, 0.3, 0.5)
        found = pin_wnms.identify(ext.wnms_gpu, DEV)
    wk, wo, wc = _want_list("no_classes", flags)
    assert np.array_equal(keep, wk) and np.array_equal(count, wc) and out.tobytes() == wo.tobytes()
    assert found == [s]
    keep, out, count = pin_wnms.run(ext.wnms_gpu, DEV, b, d, 0.3, 0.5)  # after the block: the declaration
    wk, wo, wc = _want_list("no_classes", 0)
    assert np.array_equal(keep, wk) and np.array_equal(count, wc) and out.tobytes() == wo.tobytes()


def test_shim_outside_any_block_is_the_declaration():
    ext = _shim()
    assert pin_wnms.identify(ext.wnms_gpu, DEV) == [ref.WnmsSemantics()]
    with ext.semantics(ref.WnmsSemantics(score="KEEPER")):
        with ext.semantics(ref.WnmsSemantics(merge_set="ALL")):
            assert pin_wnms.identify(ext.wnms_gpu, DEV) == [ref.WnmsSemantics(merge_set="ALL")]
        assert pin_wnms.identify(ext.wnms_gpu, DEV) == [ref.WnmsSemantics(score="KEEPER")]
    assert pin_wnms.identify(ext.wnms_gpu, DEV) == [ref.WnmsSemantics()]


def test_errors():
    hnms = _hnms()
    L = hnms.L
    b, d, _ = ref.random_list(64, 164)
    bt, dt = torch.from_numpy(b).to(DEV), torch.from_numpy(d).to(DEV)
    out, keep, count = torch.zeros_like(dt), torch.zeros(64, dtype=torch.long, device=DEV), torch.zeros(64, dtype=torch.long, device=DEV)
    ws = torch.empty(L.load().rv_wnms_workspace_bytes(64), dtype=torch.uint8, device=DEV)
    num = L.i64(0)
    with pytest.raises(L.RvError, match="unknown flag bits 0x10"):
        L.call("rv_wnms_opt", L.ptr(bt), L.ptr(dt), None, 64, 9, 0.3, 0.5, L.ptr(out), L.ptr(keep), L.ptr(count), L.ptr(ws),
               ctypes.byref(num), L.stream_ptr(), 16)
    assert not out.any()  # nothing ran

    class Bad:
        flags = 32

    orig = hnms._flags
    hnms._flags = lambda s: 32 if isinstance(s, Bad) else orig(s)
    try:
        with pytest.raises(L.RvError, match="unknown flag bits 0x20"):
            _device_batch(Bad())
    finally:
        hnms._flags = orig
    cub, sc, ct = _sweeps()
    with pytest.raises(L.RvError, match="HARD"):
        hnms.batched_multiclass_nms(cub.to(DEV), sc.to(DEV), ct.to(DEV), PRE, POST, 0.3, 0.1, "HARD", n_classes=3, semantics=ref.WnmsSemantics(score="KEEPER"))
    hard = hnms.batched_multiclass_nms(cub.to(DEV), sc.to(DEV), ct.to(DEV), PRE, POST, 0.3, 0.1, "HARD", n_classes=3, semantics=ref.WnmsSemantics())
    assert hard[0].shape[0] > 0  # the default setting is no option
    with pytest.raises(L.RvError, match="merge_compare"):
        ref.WnmsSemantics(merge_compare="EQ")
