"""Soft target assignment with every option of ``targets_config``, host side: the fixtures of ``tests/golden/assignment/`` (the reference's
own ``compute_classification_targets`` and ``DetectionHead.loss``, written by ``tests/golden/make_golden_assignment.py``) against a
plain-torch restatement of the per-instance affinity and of the top-k threshold rule.

The restatement (``restate_affinity``, ``restate_loss``) is written here and vectorised over pixels (segments by panoptic id), so
tests/test_gpu_assignment.py uses it as the yardstick at full size, where no fixture exists.  Tie rule, as ``include/rv3d.h`` declares
it: a pixel stays iff its affinity is >= the instance's ``min(k, |set|)``-th largest affinity, and != 0.
"""

from __future__ import annotations

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nms as onms
from oracle import targets as otgt
from oracle.decode import decode_range_view
from test_host_cpu import _gfx950_code_objects, _kernel_metadata
from test_multilevel_golden import LOSS_KEYS
from test_oracle_golden import GOLDEN, unpack

INF = math.inf
# the cases of tests/golden/make_golden_assignment.py (kept equal to its CASES by test_case_table_is_the_generators)
CASES = {
    "A": dict(strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="GAUSSIAN", normalize=False, k=4),
    "B": dict(strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="GAUSSIAN", normalize=True, k=INF),
    "C": dict(strides=[1], classes=[3], method=None, partitions={1: [0.0, INF]}, affinity_fn="GAUSSIAN", normalize=True, k=16),
    "D": dict(strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="BEV", normalize=False, k=INF),
    "E": dict(strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="BEV", normalize=False, k=8),
    "F": dict(strides=[1, 2], classes=[2, 1], method="RANGE", partitions={1: [0.0, 10.0], 2: [10.0, INF]}, affinity_fn="GAUSSIAN", normalize=False, k=4),
}
HAVE_REFERENCE = os.path.isdir("/root/reference/src/torchbox3d")
NEW_ENTRIES = ("rv_soft_assign_workspace_bytes", "rv_soft_assign", "rv_detection_loss_multilevel_forward_aff", "rv_detection_loss_multilevel_backward_aff")
NEW_KERNELS = ("sa_affinity_kernelILb0ELb0", "sa_affinity_kernelILb0ELb1", "sa_affinity_kernelILb1ELb0", "sa_normalize_kernel", "sa_hist_kernel",
               "sa_scan_kernel", "sa_apply_kernel", "loss_table_aff_kernelILb0", "loss_table_aff_kernelILb1")


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
def bev_iou(pds, gts):
    """Rotated BEV IoU of matching rows of two (N,7) cuboid tables, clamped to [0, 1]: ``oracle.nms.pairwise_iou`` on fp32 boxes
    ``[x - l/2, y - w/2, x + l/2, y + w/2, yaw]``, the diagonal of blocks of 64 pairs."""
    def corners(c):
        c = c.float().numpy()
        hl, hw = np.float32(0.5) * c[:, 3], np.float32(0.5) * c[:, 4]
        return np.stack([c[:, 0] - hl, c[:, 1] - hw, c[:, 0] + hl, c[:, 1] + hw, c[:, 6]], axis=1)

    a, b = corners(pds), corners(gts)
    out = np.zeros(a.shape[0], dtype=np.float32)
    for i in range(0, a.shape[0], 64):
        out[i:i + 64] = np.diagonal(onms.pairwise_iou(a[i:i + 64], b[i:i + 64]))
    return torch.from_numpy(out).clamp(0.0, 1.0)


def restate_affinity(regressands, targets, cart, affinity_fn="GAUSSIAN", normalize=False, k=INF, sigma=0.75, azimuth_invariant=True):
    """The affinity map (B,1,H,W) of ``compute_classification_targets`` (assignment.py:76-147) before ``* one_hot(labels)``: per instance
    (sweep, panoptic id >= 1; ``mask`` plays no part) the GAUSSIAN or BEV affinity, the instance minimum under ``normalize``, and the
    threshold of the top k."""
    pan = targets["panoptics"].reshape(cart.shape[0], -1)
    B, n_pix = pan.shape
    pds = decode_range_view(regressands.detach(), cart, True).flatten(2).permute(0, 2, 1)
    gts = decode_range_view(targets["regression_targets"], cart, azimuth_invariant).flatten(2).permute(0, 2, 1)
    where = (pan > 0).nonzero()
    out = torch.zeros(B, n_pix, dtype=regressands.dtype)
    if where.shape[0] == 0:
        return out.view(B, 1, *cart.shape[2:])
    b, pix = where[:, 0], where[:, 1]
    seg = b * (int(pan.max()) + 1) + pan[b, pix]  # one key per instance
    _, seg = seg.unique(return_inverse=True)
    n_seg = int(seg.max()) + 1
    if affinity_fn.upper() == "BEV":
        a = bev_iou(pds[b, pix], gts[b, pix]).to(regressands.dtype)
    else:
        d = torch.linalg.norm(pds[b, pix, :3] - gts[b, pix, :3], dim=-1)
        if normalize:
            d = d - torch.full((n_seg,), INF, dtype=d.dtype).scatter_reduce(0, seg, d, "amin")[seg]
        a = torch.exp(-d / sigma**2)
    if k != INF:
        order = a.argsort(descending=True, stable=True)
        order = order[seg[order].argsort(stable=True)]  # by instance, affinities descending within one
        count = torch.bincount(seg, minlength=n_seg)
        start = count.cumsum(0) - count
        kth = a[order][start + count.clamp(max=int(k)) - 1]  # the min(k, |set|)-th largest of every instance
        a = torch.where(a >= kth[seg], a, torch.zeros_like(a))
    out[b, pix] = a
    return out.view(B, 1, *cart.shape[2:])


def restate_loss(entries, strides, opts, additive_smoothing=1.0, sigma=0.75, alpha=0.75, gamma=2.0):
    """The dict of ``DetectionHead.loss`` + ``reduce_multiscale_loss`` with the soft targets of ``restate_affinity``; as
    ``test_multilevel_golden.restate_loss`` otherwise.  Also returns per entry (soft targets, foreground)."""
    parts, maps = [], []
    for e in entries:
        aff = restate_affinity(e["regressands"], e["targets"], e["cart"], opts["affinity_fn"], opts["normalize"], opts["k"], sigma)
        one_hot = F.one_hot(e["targets"]["classification_labels"], e["n_cls"] + 1).permute(0, 3, 1, 2)[:, :-1].to(aff.dtype)
        soft, fg = aff * one_hot, (aff != 0).to(aff.dtype)
        bg = torch.logical_and(fg.logical_not(), e["mask"])
        cls = otgt.varifocal_loss(e["logits"], soft, alpha, gamma) * e["mask"]
        norm = (e["targets"]["points_per_obj"] + additive_smoothing).double().reciprocal()
        reg = F.l1_loss(e["regressands"], e["targets"]["regression_targets"], reduction="none") * one_hot.any(dim=1, keepdim=True) * norm * e["mask"] / 8
        n_obj = sum(int((x.unique() > 0).sum()) for x in e["targets"]["panoptics"])
        parts.append((cls.double(), reg, fg, bg, n_obj))
        maps.append((soft, fg))
    total_fg = sum(float(p[2].sum()) for p in parts) + additive_smoothing
    total_objects = max(sum(p[4] for p in parts), 1)
    rows = []
    for cls, reg, fg, bg, _ in parts:
        cls = cls / total_fg
        per = (reg / total_objects).sum(dim=[0, 2, 3])
        coord, dim, rot = per[:3].sum(), per[3:6].sum(), per[6:].sum()
        rows.append({"loss": cls.sum() + coord + dim + rot, "classification_loss": cls.sum(), "foreground_loss": (cls * fg).sum(),
                     "background_loss": (cls * bg).sum(), "regression_loss": coord + dim + rot, "coordinate_loss": coord, "dimension_loss": dim,
                     "rotation_loss": rot, "total_fg": total_fg, "total_objects": float(total_objects)})
    losses = {k: sum(float(r[k]) for r in rows) for k in LOSS_KEYS}
    for k in LOSS_KEYS:
        for i, s in enumerate(strides):
            losses[f"{k}/s{s}"] = float(rows[i][k])
    return losses, maps


# ------------------------------------------------------------------------------------------------------------------
# fixture access (shared with tests/test_gpu_assignment.py)
# ------------------------------------------------------------------------------------------------------------------
def case_entries(g0, g, name):
    """The fixture's (level, task) entries in the reference's list order, tensors as the reference produced them."""
    case = CASES[name]
    entries = []
    for s in case["strides"]:
        for t, n_cls in enumerate(case["classes"]):
            p = f"s{s}/t{t}"
            tg = {k: g[f"{p}/{k}"] for k in ("classification_labels", "panoptics", "regression_targets", "points_per_obj")}
            entries.append({"stride": s, "task": t, "n_cls": n_cls, "logits": g[f"{p}/logits"], "regressands": g[f"{p}/regressands"],
                            "cart": g0["cart"][:, :, :, ::s].contiguous(), "mask": g[f"s{s}/mask"], "targets": tg, "prefix": p})
    return entries


def targets_config(name):
    case = CASES[name]
    tasks = {t: [f"T{t}C{i}" for i in range(n)] for t, n in enumerate(case["classes"])}
    tcfg = {"dataset_name": "av2", "tasks": tasks, "enable_azimuth_invariant_targets": True,
            "range_partitions": {s: case["partitions"][s] for s in case["strides"]}, "fpn_assignment_method": case["method"], "k": case["k"],
            "affinity_fn": case["affinity_fn"], "normalize_affinities": case["normalize"], "sigma": 0.75}
    return tasks, tcfg


def build_head(name, **overrides):
    from range_view_3d_detection_amd.nn.heads.detection_head import DetectionHead

    tasks, tcfg = targets_config(name)
    tcfg.update(overrides)
    fpn = {s: 32 for s in CASES[name]["strides"]}
    return DetectionHead(fpn=fpn, fpn_kernel_sizes={s: [3, 3] for s in fpn}, targets_config=tcfg, num_classification_blocks=1,
                         num_regression_blocks=1, final_kernel_size=1, tasks_cfg=tasks, task_in_channels=32, classification_weight=1.0,
                         regression_weight=1.0, coding_weights=[1.0] * 8, classification_head_channels=32, regression_head_channels=32,
                         classification_normalization_method="FOREGROUND",
                         _cls_loss={"_target_": "torchbox3d.nn.losses.classification.VarifocalLoss", "alpha": 0.75, "gamma": 2.0, "reduction": "none"},
                         _regression_loss={"_target_": "torch.nn.L1Loss", "reduction": "none"})


def instance_sets(pan):
    """(sweep, flat pixel indices) of every instance of a panoptic map."""
    flat = pan.reshape(pan.shape[0], -1)
    return [(b, (flat[b] == p).nonzero().flatten()) for b in range(flat.shape[0]) for p in flat[b].unique().tolist() if p > 0]


# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: regenerating the fixtures runs the reference")
def test_generator_reproduces_the_committed_directory(tmp_path):
    """Byte for byte, natively and on ATen's scalar code paths with one thread (see tests/test_multilevel_golden.py)."""
    names = sorted(os.listdir(os.path.join(GOLDEN, "assignment")))
    assert names == [f"{c}.npz" for c in CASES]
    assert sum(os.path.getsize(os.path.join(GOLDEN, "assignment", f)) for f in names) < 600 * 1024
    for tag, extra in (("native", {}), ("scalar", {"ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1"})):
        out_dir = tmp_path / tag
        out_dir.mkdir()
        env = dict(os.environ, RV3D_GOLDEN_OUT=str(out_dir), PYTORCH_JIT="0", **extra)
        out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_assignment.py")], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        for f in names:
            assert open(os.path.join(GOLDEN, "assignment", f), "rb").read() == open(out_dir / "assignment" / f, "rb").read(), f"{f} is not reproduced ({tag})"


@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: imports the generator, which imports the reference")
def test_case_table_is_the_generators():
    import json

    fields = ("strides", "classes", "method", "partitions", "affinity_fn", "normalize", "k")
    code = ("import sys, json; sys.path.insert(0, %r); import make_golden_assignment as m; "
            "print(json.dumps({k: {f: v[f] for f in %r} for k, v in m.CASES.items()}))" % (GOLDEN, fields))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTORCH_JIT="0"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(CASES))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_fixture(golden, name):
    """Foreground masks exactly, soft targets and every scalar of the loss dict to 1e-6."""
    g0, g, case = golden("multilevel/common"), golden(f"assignment/{name}"), CASES[name]
    entries = case_entries(g0, g, name)
    losses, maps = restate_loss(entries, case["strides"], case)
    ref = unpack(g, "loss")
    assert set(ref) == set(losses)
    for k, v in ref.items():
        assert abs(losses[k] - float(v)) <= 1e-6 * max(1.0, abs(float(v))), (name, k, losses[k], float(v))
    for e, (soft, fg) in zip(entries, maps):
        assert torch.equal(fg, g[f"{e['prefix']}/foreground"]), (name, e["prefix"])
        assert torch.allclose(soft, g[f"{e['prefix']}/soft"], atol=1e-6), (name, e["prefix"])


def test_fixtures_hold_what_the_cases_are_for(golden):
    """The situations the cases exist for, read from the stored tensors (the generator asserts them too, on the reference's run)."""
    g0 = golden("multilevel/common")

    def per_instance(name, p="s1/t0"):
        g = golden(f"assignment/{name}")
        fg, soft = g[f"{p}/foreground"].reshape(2, -1), g[f"{p}/soft"].sum(dim=1).reshape(2, -1)
        return g, [(b, idx, int(fg[b, idx].sum()), soft[b, idx]) for b, idx in instance_sets(g[f"{p}/panoptics"])]

    a, inst = per_instance("A")
    sizes = [idx.numel() for _, idx, _, _ in inst]
    assert min(sizes) < 4 and 4 in sizes and max(sizes) > 8 and all(n == min(4, idx.numel()) for _, idx, n, _ in inst)
    assert int(a["s1/t0/panoptics"][1].max()) == 0 and not (a["annotations"][:, 12] == 1).any()
    # a pixel with mask == 0 (its geometry is valid: the common sweep's mask has it) inside an instance's set and inside its top 4
    extra = (g0["mask"] & ~a["mask"]).reshape(2, -1).nonzero()
    assert extra.shape[0] == 1
    b, pix = extra[0].tolist()
    assert int(a["s1/t0/panoptics"].reshape(2, -1)[b, pix]) > 0 and float(a["s1/t0/foreground"].reshape(2, -1)[b, pix]) == 1.0
    for name in ("B", "C"):  # normalised: the best pixel of every instance has affinity exactly 1
        _, inst = per_instance(name)
        assert inst and all(float(s.max()) == 1.0 for _, _, _, s in inst)
    _, inst = per_instance("C")
    assert any(idx.numel() > 16 for _, idx, _, _ in inst) and all(n == min(16, idx.numel()) for _, idx, n, _ in inst)
    _, inst = per_instance("D")  # BEV: an IoU of 0 is not foreground, k = inf or not
    assert any(0 < n < idx.numel() for _, idx, n, _ in inst) and any(n == 0 for _, _, n, _ in inst)
    _, inst = per_instance("E")
    assert any(idx.numel() > 8 for _, idx, _, _ in inst) and all(n <= 8 for _, _, n, _ in inst)
    f = golden("assignment/F")
    for p in ("s1/t0", "s1/t1", "s2/t0", "s2/t1"):  # the selection is per (level, task, sweep, instance)
        _, inst = per_instance("F", p)
        assert inst and all(n == min(4, idx.numel()) for _, idx, n, _ in inst), p
    assert not torch.equal(f["s1/mask"], g0["mask"])  # the RANGE partition is in the stored mask


def test_the_threshold_rule_on_constructed_ties():
    """All affinities equal: ``k = 3`` keeps every pixel.  Two groups straddling the k-th place: the whole lower group stays."""
    cart = torch.zeros(1, 3, 1, 8)
    cart[0, 0] = 5.0
    tg = {"panoptics": torch.tensor([1, 1, 1, 1, 1, 2, 2, 0]).view(1, 1, 1, 8), "regression_targets": torch.zeros(1, 8, 1, 8)}
    reg = torch.zeros(1, 8, 1, 8)
    reg[0, 0, 0] = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0.25, 1.0, 0.1])
    aff = restate_affinity(reg, tg, cart, k=3).flatten()
    assert (aff[:5] != 0).all() and aff[5] != 0 and aff[6] != 0 and aff[7] == 0
    reg[0, 0, 0, :5] = torch.tensor([0.25, 0.25, 0.5, 0.5, 0.5])
    aff = restate_affinity(reg, tg, cart, k=3).flatten()
    assert int((aff[:5] != 0).sum()) == 5
    reg[0, 0, 0, :5] = torch.tensor([0.25, 0.25, 0.25, 0.5, 0.5])
    assert int((restate_affinity(reg, tg, cart, k=3).flatten()[:5] != 0).sum()) == 3


def test_option_parsing():
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.nn.heads import detection_head as dh

    assert dh.soft_options({}) == (L.AFFINITY_GAUSSIAN, False, 0) and dh._soft_is_default(dh.soft_options({"affinity_fn": "gaussian", "k": INF}))
    assert dh.soft_options({"affinity_fn": "bev", "k": 8.0}) == (L.AFFINITY_BEV, False, 8)
    assert dh.soft_options({"normalize_affinities": True, "k": 16}) == (L.AFFINITY_GAUSSIAN, True, 16)
    with pytest.raises(ValueError, match=r"assignment\.py:71-72"):
        dh.soft_options({"affinity_fn": "BEV", "normalize_affinities": True})
    for bad in (0, 2.5, -1, float("nan"), "4"):
        with pytest.raises(ValueError, match="k must be"):
            dh.soft_options({"k": bad})
    with pytest.raises(NotImplementedError, match="This affinity function is not implemented."):
        dh.soft_options({"affinity_fn": "iou_3d_axis_aligned"})


def test_new_entries_are_declared_and_exported():
    from range_view_3d_detection_amd import _lib

    assert set(NEW_ENTRIES) <= set(_lib.declared_symbols())
    for tag in ("bf16", "f16"):
        lib = _lib.load(tag)
        assert all(hasattr(lib, n) for n in NEW_ENTRIES)
        # 259 u32 per slot, n_entries * (m + B) slots, rounded up to 256 bytes
        assert lib.rv_soft_assign_workspace_bytes(2, 10, 4) == 2 * 14 * 259 * 4 + (-2 * 14 * 259 * 4) % 256
        assert lib.rv_soft_assign_workspace_bytes(0, 10, 4) == 0
    header = open(_lib.HEADER_PATH).read()
    assert "assignment.py:76-147" in header and "k_actual-th largest" in header


@pytest.mark.parametrize("path_attr", ["LIB_PATH", "LIB_PATH_F16"])
def test_new_kernels_do_not_spill(tmp_path, path_attr):
    """No VGPR spills in the soft-assignment kernels and in the loss kernels that read the maps.  The BEV affinity kernel indexes the
    clip polygons of ``nms_geom.h`` (two arrays of 16 points) dynamically, so it owns a private segment, as the NMS kernels do: that
    is not a spill, and only there is it allowed."""
    from range_view_3d_detection_amd import _lib

    found = set()
    for i, co in enumerate(_gfx950_code_objects(getattr(_lib, path_attr))):
        if b"sa_scan_kernel" not in co and b"loss_table_aff_kernel" not in co:
            continue
        path = tmp_path / f"{i}.co"
        path.write_bytes(co)
        for name in NEW_KERNELS:
            if name.encode() in co:
                md = _kernel_metadata(path, name)
                assert int(md["vgpr_spill_count"]) == 0, md
                assert int(md["private_segment_fixed_size"]) == 0 or name == "sa_affinity_kernelILb1ELb0", md
                found.add(name)
    assert found == set(NEW_KERNELS)
