"""``nms_mode: HARD``, host side: the fixtures of ``tests/golden/nms_hard/`` (the reference's own ``hard_multiclass_nms``,
``batched_multiclass_nms(nms_mode="HARD")`` and ``RangeDecoder.decode`` over a ``nms_rotated`` stand-in, written by
``tests/golden/make_golden_nms_hard.py``) against the numpy restatement of the declared semantics (``tests/nms_hard_ref.py``), which
tests/test_gpu_nms_hard.py uses as the yardstick where no fixture exists.
"""

from __future__ import annotations

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nms_hard_ref as ref
from nms_hard_ref import same_rows_exact
from oracle import decode as odec
from test_oracle_golden import GOLDEN

HAVE_REFERENCE = os.path.isdir("/root/reference/src/torchbox3d")
TAGS = ("post1000", "post40", "pre150")
NEW_ENTRIES = ("rv_nms_rotated_workspace_bytes", "rv_nms_rotated", "rv_nms_sweeps_hard")


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_fixture(golden, tag):
    g = golden("nms_hard/wrapper")
    pre, post, thr, conf = g.np(f"a/{tag}/cfg").tolist()
    got = ref.batched_rows(g["a/cuboids"], g["a/scores"], g["a/categories"], int(pre), int(post), thr, conf)
    same_rows_exact(got, tuple(g[f"a/{tag}/{k}"] for k in ("params", "scores", "categories", "batch_index")), tag)


def test_restatement_equals_the_fixture_one_sweep_chain_and_empty(golden):
    g = golden("nms_hard/wrapper")
    cub, sc, cat = g["a/cuboids"], g["a/scores"], g["a/categories"]
    m = sc[0] >= 0.1
    rows, classes = ref.hard_multiclass(cub[0, m].numpy(), sc[0, m].numpy(), cat[0, m].numpy(), 0.3, 50000, 40)
    zero = torch.zeros(len(rows))
    same_rows_exact((cub[0, m][rows], sc[0, m][rows], torch.from_numpy(classes).float(), zero),
                    (g["a/multiclass/params"], g["a/multiclass/scores"], g["a/multiclass/categories"], zero), "hard_multiclass_nms")
    got = ref.batched_rows(g["c/cuboids"], g["c/scores"], g["c/categories"], 50000, 1000, 0.3, 0.1)
    same_rows_exact(got, (g["c/params"], g["c/scores_out"], g["c/categories_out"], g["c/batch_index"]), "chain")
    p, s, c, b = ref.batched_rows(cub[1:2], sc[1:2], cat[1:2], 50000, 1000, 0.3, 0.1)
    assert list(p.shape) == g.np("a/empty/params_shape").tolist() and list(s.shape) == g.np("a/empty/scores_shape").tolist()
    assert list(c.shape) == g.np("a/empty/categories_shape").tolist() and list(b.shape) == g.np("a/empty/batch_index_shape").tolist()
    assert (c.dtype == torch.int64) == bool(g.np("a/empty/categories_is_int64"))


def test_fixtures_hold_what_the_cases_are_for(golden):
    """Read from the stored tensors (the generator asserts them too, on the reference's run)."""
    g = golden("nms_hard/wrapper")
    cub, sc, cat = g["a/cuboids"], g["a/scores"], g["a/categories"]
    live = sc >= 0.1
    assert not bool((cat == 3).any()) and int(live[1].sum()) == 0
    assert int((live[0] & (cat[0] == 1)).sum()) > 0.4 * int(live[0].sum()) > 150
    s2 = sc[2][live[2]]
    assert len(s2.unique()) < len(s2) - 60  # exact score ties
    assert int(g["a/pre150/params"].shape[0]) < int(g["a/post1000/params"].shape[0])  # the pre-NMS cut bites
    per_class = [int(((g["a/post40/categories"] == j) & (g["a/post40/batch_index"] == 0)).sum()) for j in range(5)]
    assert per_class == [40, 40, 40, 0, 40]  # the post-NMS cut bites
    # every stored row is an input row, bit for bit
    rows = {r.numpy().tobytes() for r in cub.reshape(-1, 7)}
    assert all(r.numpy().tobytes() in rows for r in g["a/post1000/params"])
    # the chain sits at sorted positions 63 / 64 / 65 of class 0; IoU(A,B), IoU(B,C) above the threshold, IoU(A,C) below
    c_cub, c_sc, c_cat = g["c/cuboids"][0], g["c/scores"][0], g["c/categories"][0]
    idx0 = (c_cat == 0).nonzero().flatten()
    order = idx0[torch.from_numpy(ref.score_order(c_sc[idx0].numpy()))]
    assert torch.equal(c_cub[order[63:66]], g["c/chain"])
    iou = ref.onms.pairwise_iou(ref.rect_of(g["c/chain"].numpy()), ref.rect_of(g["c/chain"].numpy()))
    assert iou[0, 1] > 0.3 and iou[1, 2] > 0.3 and iou[0, 2] < 0.3
    out0 = g["c/params"][g["c/categories_out"] == 0]
    has = lambda r: bool((out0 == r).all(dim=1).any())  # noqa: E731
    assert has(g["c/chain"][0]) and not has(g["c/chain"][1]) and has(g["c/chain"][2])


@pytest.mark.parametrize("tag,sample", [("tiny", True), ("sampled", True), ("dense", False)])
def test_restated_decode_equals_the_fixture(golden, tag, sample):
    """``RangeDecoder.decode(use_nms=True)`` HARD: the oracle's candidates, the restated NMS, the quaternion columns."""
    g = golden("nms_hard/decode")
    t = golden("tiny_model") if tag == "tiny" else golden("decode")
    logits, reg = (t["eval/logits"], t["eval/regressands"]) if tag == "tiny" else (t["logits"], t["regressands"])
    s, c, b = odec.dense_candidates(logits, reg, t["cart"], t["mask"], enable_sample_by_range=sample)
    p, s, c, bi = ref.batched_rows(b, s, c, 50000, int(g.np(f"b/{tag}/num_post_nms")), 0.3, 0.1)
    p = torch.cat([p[:, :-1], odec.yaw_to_quat(p[:, -1:])], dim=-1)
    want = tuple(g[f"b/{tag}/{k}"] for k in ("params", "scores", "categories", "batch_index"))
    assert p.shape == want[0].shape and p.shape[1] == 10
    assert torch.equal(c, want[2]) and torch.equal(bi, want[3])
    assert torch.allclose(p, want[0], atol=1e-5) and torch.allclose(s, want[1], atol=1e-6)


@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: regenerating the fixtures runs the reference")
def test_generator_reproduces_the_committed_directory(tmp_path):
    """Byte for byte; ``wrapper.npz`` also on ATen's scalar code paths with one thread (``decode.npz`` holds the reference's fp32
    sigmoid, as ``nms_wrapper.npz`` does)."""
    names = sorted(os.listdir(os.path.join(GOLDEN, "nms_hard")))
    assert names == ["decode.npz", "wrapper.npz"]
    assert sum(os.path.getsize(os.path.join(GOLDEN, "nms_hard", f)) for f in names) < 400 * 1024
    for tag, extra, files in (("native", {}, names), ("scalar", {"ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1"}, ["wrapper.npz"])):
        out_dir = tmp_path / tag
        out_dir.mkdir()
        env = dict(os.environ, RV3D_GOLDEN_OUT=str(out_dir), PYTORCH_JIT="0", **extra)
        out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_nms_hard.py")], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        for f in files:
            assert open(os.path.join(GOLDEN, "nms_hard", f), "rb").read() == open(out_dir / "nms_hard" / f, "rb").read(), f"{f} is not reproduced ({tag})"


def test_restated_nms_rotated_has_detectron2s_contract():
    """Unsorted (cx, cy, w, h, degrees): indices in descending score order, ties by ascending index, strictly-greater rule."""
    boxes = np.array([[0, 0, 4, 2, 0], [1, 0, 4, 2, 0], [0, 0, 4, 2, 90], [10, 0, 4, 2, 0], [10, 0, 4, 2, 0]], dtype=np.float32)
    scores = np.array([0.5, 0.9, 0.5, 0.25, 0.25], dtype=np.float32)
    # box 1 first; IoU(1, 0) = 0.6 suppresses 0 at 0.5; box 2 (IoU with 1 = 2 / 14) stays; 3 before 4 (tie), IoU 1 suppresses 4
    assert ref.nms_rotated(boxes, scores, 0.5).tolist() == [1, 2, 3]
    assert ref.nms_rotated(boxes, scores, 0.6).tolist() == [1, 0, 2, 3]  # IoU == threshold does not suppress (3 / 5 in fp32 both ways)
    assert ref.nms_rotated(boxes[:0], scores[:0], 0.5).tolist() == []


def test_nms_rotated_shim_importable_and_refuses_cpu_tensors():
    """``compat/detectron2_nms.py`` imports without a GPU; there is no CPU fallback."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.compat.detectron2_nms import nms_rotated

    with pytest.raises(L.RvError, match="GPU"):
        nms_rotated(torch.zeros(4, 5), torch.zeros(4), 0.3)
    with pytest.raises(L.RvError, match="GPU"):
        nms_rotated(boxes=torch.zeros(4, 5), scores=torch.zeros(4), iou_threshold=torch.as_tensor(0.3))


def test_unknown_mode_message_and_known_modes():
    from range_view_3d_detection_amd.math.ops import nms as hnms

    z = torch.zeros(1, 4, 7), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="NMS Mode: SOFT is not implemented."):
        hnms.batched_multiclass_nms(*z, 10, 10, 0.3, 0.1, "soft", n_classes=2)
    for mode in ("HARD", "hard", "Weighted"):
        with pytest.raises(RuntimeError) as e:  # past the mode check: refused for being CPU tensors
            hnms.batched_multiclass_nms(*z, 10, 10, 0.3, 0.1, mode, n_classes=2)
        assert not isinstance(e.value, NotImplementedError)


def test_both_libraries_export_the_hard_entries_and_kernels():
    from range_view_3d_detection_amd import _lib as L
    from test_host_cpu import _gfx950_code_objects

    assert set(NEW_ENTRIES) <= set(L.declared_symbols())
    for tag, path in (("bf16", L.LIB_PATH), ("f16", L.LIB_PATH_F16)):
        lib = L.load(tag)
        assert all(hasattr(lib, n) for n in NEW_ENTRIES), tag
        assert lib.rv_nms_rotated_workspace_bytes(1000) >= 1000 * 16 * 8 + 1000 * 8
        blob = b"".join(_gfx950_code_objects(path))
        for kernel in (b"k_post_hard", b"k_scanILb1E", b"k_iouILb1E", b"k_gatherILb1E", b"scan_kernelILb1E", b"iou_mask_kernelILb1E",
                       b"k_scanILb0E", b"k_iouILb0E", b"scan_kernelILb0E"):
            assert kernel in blob, (tag, kernel)
