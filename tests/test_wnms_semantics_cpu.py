"""The weighted-NMS choices (``WnmsSemantics``) without a GPU: the option type, the numpy restatement of all 16 settings
(``tests/wnms_semantics_ref.py``) against the oracle and on hand-built lists, and the pin tool (``tests/tools/pin_wnms.py``)."""

from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wnms_semantics_ref as ref
from oracle import nms as onms
from range_view_3d_detection_amd._lib import RvError
from range_view_3d_detection_amd.math.ops import nms as hnms
from range_view_3d_detection_amd.math.ops.nms import WnmsSemantics

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import pin_wnms  # noqa: E402

sys.path.pop(0)

DEFAULT = WnmsSemantics()


def _sem(**kw):
    return WnmsSemantics(**kw)


def test_option_type_flags_and_config():
    assert DEFAULT.flags == 0 and len(set(s.flags for s in ref.ALL_SETTINGS)) == 16
    assert _sem(merge_set="ALL").flags == 1 and _sem(score="KEEPER").flags == 2 and _sem(nms_compare="GE").flags == 4
    assert _sem(merge_compare="GE").flags == 8 and _sem(merge_set="all", score="keeper", nms_compare="ge", merge_compare="ge").flags == 15
    for s in ref.ALL_SETTINGS:
        assert WnmsSemantics.from_flags(s.flags) == s
        assert WnmsSemantics.from_config({"merge_set": s.merge_set, "score": s.score, "nms_compare": s.nms_compare, "merge_compare": s.merge_compare}) == s
    assert WnmsSemantics.from_config(None) == DEFAULT and WnmsSemantics.from_config({}) == DEFAULT
    assert WnmsSemantics.from_config({"score": "KEEPER"}) == _sem(score="KEEPER")
    with pytest.raises(Exception):  # frozen
        DEFAULT.score = "KEEPER"
    with pytest.raises(RvError, match="merge_sett"):
        WnmsSemantics.from_config({"merge_sett": "ALL"})
    with pytest.raises(RvError, match="SOMETIMES"):
        WnmsSemantics.from_config({"merge_set": "SOMETIMES"})
    with pytest.raises(RvError, match="nms_compare"):
        WnmsSemantics(nms_compare="LT")


def test_option_type_from_an_omegaconf_mapping():
    OmegaConf = pytest.importorskip("omegaconf").OmegaConf
    cfg = OmegaConf.create({"post": {"wnms_semantics": {"merge_set": "ALL", "merge_compare": "GE"}}})
    assert WnmsSemantics.from_config(cfg.post.wnms_semantics) == _sem(merge_set="ALL", merge_compare="GE")
    with pytest.raises(RvError, match="scor"):
        WnmsSemantics.from_config(OmegaConf.create({"scor": "MEAN"}))


def test_hard_mode_takes_no_semantics():
    """Raised before anything touches a device."""
    z = torch.zeros(1, 4, 7)
    with pytest.raises(RvError, match="HARD"):
        hnms.batched_multiclass_nms(z, torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.long), 10, 10, 0.3, 0.1, "HARD", n_classes=2,
                                    semantics=_sem(score="KEEPER"))
    with pytest.raises(RvError, match="HARD"):
        hnms.nms_sweeps(z, torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.long), 2, 0.3, 0.1, 10, 64, mode="HARD", semantics=_sem(nms_compare="GE"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 200])
def test_default_restatement_equals_the_oracle_bit_for_bit(n):
    b, d, _ = ref.random_list(n, 100 + n)
    bt, dt = torch.from_numpy(b), torch.from_numpy(d)
    keep, out, count = onms.weighted_nms(bt, dt[:, :-1], dt[:, -1], 0.3, 0.5)
    rk, ro, rc = ref.weighted_nms(bt, dt[:, :-1], dt[:, -1], 0.3, 0.5, DEFAULT)
    assert torch.equal(keep, rk) and torch.equal(count, rc) and torch.equal(out, ro)
    if n >= 130:
        assert int(count.max()) >= 3 and len(keep) < n  # the list does cluster


def test_default_restatement_equals_the_oracle_on_rotated_sweeps():
    cub, sc, ct = ref.sweeps()
    want = onms.batched_multiclass_nms(cub, sc, ct, 100, 20, 0.3, 0.1)
    got = ref.batched_multiclass_nms(cub, sc, ct, 100, 20, 0.3, 0.1, DEFAULT)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_exact_threshold_ious_are_exact():
    """The equalities the threshold cases rest on, in the IoU arithmetic itself."""
    b, _ = ref.threshold_list()
    iou = onms.pairwise_iou(b, b)
    assert iou[0, 1] == np.float32(0.3) and iou[2, 3] == np.float32(0.5)
    off = iou[:4, :4].copy()
    off[[0, 1, 2, 3], [0, 1, 2, 3]] = 0
    off[[0, 1, 2, 3], [1, 0, 3, 2]] = 0
    assert not off.any()
    c, _ = ref.chain_list()
    ic = onms.pairwise_iou(c[[3, 70, 130]], c[[3, 70, 130]])
    assert ic[0, 2] == ic[1, 2] == np.float32(2.125) / np.float32(3.875) and ic[0, 1] == np.float32(1.25) / np.float32(4.75)
    f, _ = ref.far_list()
    assert not np.triu(onms.pairwise_iou(f, f), 1).any()


def test_merge_set_chain():
    b, d = ref.chain_list()
    for s in ref.ALL_SETTINGS:
        keep, out, count = ref.wnms_sorted(b, d, 0.3, 0.5, s)
        assert 130 not in keep and keep[3] == 3 and len(keep) == 139  # B (130) is suppressed by A (3)
        at = {int(k): int(c) for k, c in zip(keep, count)}
        assert at[3] == 2 and at[70] == (2 if s.merge_set == "ALL" else 1)  # C (70) takes the suppressed B under ALL only
        assert all(c == 1 for k, c in at.items() if k not in (3, 70))


@pytest.mark.parametrize("nms_t,merge_t", [(0.3, 0.5), (0.5, 0.5)])
def test_exact_threshold_pairs(nms_t, merge_t):
    b, d = ref.threshold_list()
    for s in ref.ALL_SETTINGS:
        keep, out, count = ref.wnms_sorted(b, d, nms_t, merge_t, s)
        at = {int(k): int(c) for k, c in zip(keep, count)}
        ge_n, ge_m = s.nms_compare == "GE", s.merge_compare == "GE"
        if nms_t == 0.3:
            assert (1 in at) == (not ge_n) and at[0] == 1  # the 0.3 pair: suppressed only under GE, never merged
            assert 3 not in at and at[2] == (2 if ge_m else 1)  # the 0.5 pair: always suppressed, merged only under GE
        else:
            assert 1 in at and at[0] == 1
            assert (3 in at) == (not ge_n)  # one pair at both thresholds: the two tests are independent
            assert at[2] == (2 if ge_m else 1)


def test_score_column():
    b, d = ref.score_list()
    for s in ref.ALL_SETTINGS:
        keep, out, count = ref.wnms_sorted(b, d, 0.3, 0.5, s)
        mean = ref.wnms_sorted(b, d, 0.3, 0.5, WnmsSemantics(s.merge_set, "MEAN", s.nms_compare, s.merge_compare))
        assert keep.tolist() == [0, 1] and count.tolist() == [3, 3]
        assert np.array_equal(out[:, :-1], mean[1][:, :-1])
        if s.score == "KEEPER":
            assert out[:, -1].tobytes() == d[[0, 1], -1].tobytes() and out[0, -1] > out[1, -1]
        else:
            assert out[0, -1] < out[1, -1] and abs(float(out[0, -1]) - 0.86 / 1.2) < 1e-6


def test_threshold_zero():
    b, d = ref.far_list()
    n = b.shape[0]
    for s in ref.ALL_SETTINGS:
        keep, out, count = ref.wnms_sorted(b, d, 0.0, 0.0, s)
        if s.nms_compare == "GE":
            assert keep.tolist() == [0] and count.tolist() == [n if s.merge_compare == "GE" else 1]
        else:
            assert keep.tolist() == list(range(n))
            # (nothing is ever suppressed, so ALIVE and ALL agree: under GE every later box is a member)
            assert count.tolist() == ([n - i for i in range(n)] if s.merge_compare == "GE" else [1] * n)


def _ref_callable(setting):
    def wnms_gpu(boxes, data, output, keep, count, nms_thresh, merge_thresh, device_index):
        k, o, c = ref.wnms_sorted(boxes.numpy(), data.numpy(), nms_thresh, merge_thresh, setting)
        n = len(k)
        keep[:n] = torch.from_numpy(k)
        output[:n] = torch.from_numpy(o)
        count[:n] = torch.from_numpy(c)
        return n

    return wnms_gpu


@pytest.mark.parametrize("flags", range(16))
def test_identify_separates_all_sixteen_settings(flags):
    s = WnmsSemantics.from_flags(flags)
    assert pin_wnms.identify(_ref_callable(s), "cpu") == [s]


def test_identify_on_a_callable_outside_the_sixteen():
    def hard(boxes, data, output, keep, count, nms_thresh, merge_thresh, device_index):  # keeps rows unmerged
        k, _, c = ref.wnms_sorted(boxes.numpy(), data.numpy(), nms_thresh, merge_thresh, DEFAULT)
        keep[: len(k)] = torch.from_numpy(k)
        output[: len(k)] = data[torch.from_numpy(k)]
        count[: len(k)] = torch.from_numpy(c)
        return len(k)

    assert pin_wnms.identify(hard, "cpu") == []


def test_pin_tool_without_torchex_says_so_and_exits_zero():
    """The tool's own command line: TorchEx is not a dependency of this project, so a top-level ``weighted_nms_ext`` is not expected."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "pin_wnms.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "no top-level weighted_nms_ext" in r.stdout and "unpinned" in r.stdout


def test_library_declares_and_rejects():
    """The two new entries are declared (``include/rv3d_wnms.h``, a part of ``include/rv3d.h``) with a trailing ``flags``, exported by
    both builds and typed by ``load()``; the library still holds no option state; an unknown bit is refused."""
    from range_view_3d_detection_amd import _lib

    protos, new = _lib.prototypes(), _lib.included_prototypes()
    assert sorted(new) == ["rv_nms_sweeps_opt", "rv_wnms_opt"] and not set(new) & set(protos)
    for name, old in (("rv_wnms_opt", "rv_wnms_classes"), ("rv_nms_sweeps_opt", "rv_nms_sweeps")):
        assert new[name][0] is ctypes.c_int32
        assert new[name][1] == protos[old][1] + ((ctypes.c_int32, "flags"),)
    header = open(_lib.HEADER_PATH).read()
    assert '#include "rv3d_wnms.h"' in header and all(f"#define RV_WNMS_{k}" in header for k in ("MERGE_SUPPRESSED", "SCORE_KEEPER", "NMS_GE", "MERGE_GE"))
    for tag in ("bf16", "f16"):
        h = _lib.load(tag)
        assert not hasattr(h, "rv_set_option")
        for name, (_, params) in new.items():
            assert len(getattr(h, name).argtypes) == len(params), (tag, name)
    h = _lib.load()
    num = _lib.i64(7)
    # an unknown bit is refused before any pointer is looked at (and before the n == 0 early return)
    assert h.rv_wnms_opt(None, None, None, 0, 9, 0.3, 0.5, None, None, None, None, ctypes.byref(num), None, 16) != 0
    assert b"flag" in h.rv_last_error() and num.value == 0
    assert h.rv_wnms_opt(None, None, None, 0, 9, 0.3, 0.5, None, None, None, None, ctypes.byref(num), None, 15) == 0


def test_a_named_but_missing_included_header_is_an_error(tmp_path, monkeypatch):
    from range_view_3d_detection_amd import _lib

    (tmp_path / "rv3d.h").write_text(open(_lib.HEADER_PATH).read())
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "rv3d.h"))
    _lib.included_prototypes.cache_clear()
    try:
        with pytest.raises(RvError, match="rv3d_wnms.h"):
            _lib.included_prototypes()
    finally:
        monkeypatch.undo()
        _lib.included_prototypes.cache_clear()
    assert len(_lib.included_prototypes()) == 2
