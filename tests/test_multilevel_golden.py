"""DetectionHead with several FPN strides and several tasks, host side: the fixtures of ``tests/golden/multilevel/`` (the reference's
own RangeNet + DetectionHead + RangeDecoder, written by ``tests/golden/make_golden_multilevel.py``) against a plain-torch restatement
of strided / range-partitioned / per-task target assignment and of the multi-level loss dict.

The restatement (``restate_targets``, ``restate_loss``) is written here, on top of the per-pixel primitives of ``oracle/targets.py``
(slab tests, target encoding, soft targets, varifocal loss: pinned to the reference by tests/test_oracle_golden.py).  It is vectorised
over pixels and boxes, so tests/test_gpu_multilevel.py uses it as the yardstick at full size, where no fixture exists.
"""

from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import targets as otgt
from test_oracle_golden import GOLDEN, unpack

INF = math.inf
# the cases of tests/golden/make_golden_multilevel.py (kept equal to its CASES by test_case_table_is_the_generators)
CASES = {
    "A": dict(strides=[1, 2, 4], classes=[2], method=None, partitions={1: [0.0, INF], 2: [0.0, INF], 4: [0.0, INF]}),
    "B": dict(strides=[1, 2, 4], classes=[2], method="RANGE", partitions={1: [0.0, 8.0], 2: [8.0, 15.0], 4: [15.0, INF]}),
    "C": dict(strides=[1], classes=[3, 2], method=None, partitions={1: [0.0, INF]}),
    "D": dict(strides=[1, 2], classes=[2, 1], method="RANGE", partitions={1: [0.0, 10.0], 2: [10.0, INF]}),
}
LEVEL_CHANNELS = {1: 16, 2: 8, 4: 16}  # what RangeNet(layers [8, 8, 16, 16, 16]) returns at strides 1, 2, 4
LOSS_KEYS = ("loss", "classification_loss", "foreground_loss", "background_loss", "regression_loss", "coordinate_loss", "dimension_loss",
             "rotation_loss", "total_fg", "total_objects")
HAVE_REFERENCE = os.path.isdir("/root/reference/src/torchbox3d")


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
def restate_targets(cart, annotations, strides, classes, method, partitions, azimuth_invariant=True):
    """{stride: {task: targets}} of ``compute_targets`` for any strides / tasks (reference: detection_head.py:496-665).

    The interior test runs once at full resolution; level ``s`` sees the columns ``::s``; RANGE keeps the annotations with
    ``lower < ||centre|| <= upper``; a task takes the rows with its id in the task column; boxes are ranked by the STRIDED interior
    count (stable, ascending) and a pixel goes to the containing box of lowest rank.  ``num_objects`` = boxes that own a pixel."""
    B, _, H, W = cart.shape
    ann = torch.as_tensor(np.asarray(annotations), dtype=torch.float64).reshape(-1, 13)
    cub = otgt.annotations_to_cuboids(ann) if ann.shape[0] else torch.zeros((0, 10), dtype=torch.float64)
    out = {}
    for s in strides:
        ws = W // s
        out[s] = {t: {"points_per_obj": torch.zeros((B, 1, H, ws), dtype=torch.int64), "panoptics": torch.zeros((B, 1, H, ws), dtype=torch.int64),
                      "classification_labels": torch.full((B, H, ws), n, dtype=torch.int64), "regression_targets": torch.zeros((B, 8, H, ws)),
                      "num_objects": 0} for t, n in enumerate(classes)}
    if cub.shape[0] == 0:
        return out
    verts = otgt.cuboids_to_vertices(cub[:, :7].float())
    dist = cub[:, :3].norm(dim=-1)
    for b in range(B):
        sel = cub[:, -1] == b
        if not bool(sel.any()):
            continue
        pts = cart[b].flatten(1, 2).t().contiguous()
        inside_full = otgt.interior_points_mask(pts.double(), verts[sel].double()).view(-1, H, W)
        for s in strides:
            inside_s = inside_full[:, :, ::s].flatten(1, 2)
            pts_s = cart[b, :, :, ::s].flatten(1, 2).t().contiguous()
            ws = W // s
            for t, n_cls in enumerate(classes):
                keep = cub[sel][:, 7].long() == t
                if method == "RANGE":
                    lower, upper = partitions[s]
                    keep &= (dist[sel] > lower) & (dist[sel] <= upper)
                if not bool(keep.any()):
                    continue
                cub_k, inside = cub[sel][keep], inside_s[keep]
                n_pts = inside.sum(dim=-1)
                _, perm = n_pts.sort(stable=True, descending=False)
                n_pts, cub_k, inside = n_pts[perm], cub_k[perm], inside[perm]
                M = inside.shape[0]
                ids = torch.where(inside, torch.arange(1, M + 1)[:, None], torch.full((1, 1), M + 1))
                winner = ids.min(dim=0).values
                fg = winner <= M
                w0 = (winner - 1).clamp(0, M - 1)
                reg = otgt.encode_regression_targets(cub_k, pts_s, azimuth_invariant)[w0, torch.arange(pts_s.shape[0])] * fg[:, None]
                tg = out[s][t]
                tg["classification_labels"][b] = torch.where(fg, cub_k[:, 8].long()[w0], torch.full_like(winner, n_cls)).view(H, ws)
                tg["panoptics"][b, 0] = torch.where(fg, winner, torch.zeros_like(winner)).view(H, ws)
                tg["regression_targets"][b] = reg.t().reshape(8, H, ws)
                tg["points_per_obj"][b, 0] = torch.where(fg, n_pts[w0], torch.zeros_like(winner)).view(H, ws)
                tg["num_objects"] += int(winner[fg].unique().numel())
    return out


def restate_loss(entries, strides, additive_smoothing=1.0, sigma=0.75, alpha=0.75, gamma=2.0):
    """The dict of ``DetectionHead.loss`` + ``reduce_multiscale_loss`` (detection_head.py:202-449) for a stride-major list of
    (level, task) ``entries`` (dicts: logits, regressands, cart, mask, targets, n_cls).  Every entry is normalised by the foreground
    count and the object count summed over ALL entries; the dict sums each scalar over the list (the two normalisers too: n x the
    value), and ``/s{stride}`` is entry ``i`` of that list for the i-th stride.  Also returns per entry (soft targets, foreground)."""
    parts, maps = [], []
    for e in entries:
        soft, fg, bg, reg_w = otgt.classification_targets(e["regressands"], e["targets"], e["cart"], e["mask"], e["n_cls"], sigma, True)
        cls = otgt.varifocal_loss(e["logits"], soft, alpha, gamma) * e["mask"]
        norm = (e["targets"]["points_per_obj"] + additive_smoothing).double().reciprocal()
        reg = F.l1_loss(e["regressands"], e["targets"]["regression_targets"], reduction="none") * reg_w * norm * e["mask"] / 8
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
                     "rotation_loss": rot, "total_fg": torch.tensor(total_fg), "total_objects": torch.tensor(float(total_objects))})
    losses = {k: sum(float(r[k]) for r in rows) for k in LOSS_KEYS}
    for k in LOSS_KEYS:
        for i, s in enumerate(strides):
            losses[f"{k}/s{s}"] = float(rows[i][k])
    return losses, maps


# ------------------------------------------------------------------------------------------------------------------
# fixture access (shared with tests/test_gpu_multilevel.py)
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


def model_config(name):
    """Constructor arguments of the case's DetectionHead (tasks, targets_config, fpn), as make_golden_multilevel.py builds it."""
    case = CASES[name]
    tasks = {t: [f"T{t}C{i}" for i in range(n)] for t, n in enumerate(case["classes"])}
    tcfg = {"dataset_name": "av2", "tasks": tasks, "enable_azimuth_invariant_targets": True,
            "range_partitions": {s: case["partitions"][s] for s in case["strides"]}, "fpn_assignment_method": case["method"], "k": INF,
            "affinity_fn": "GAUSSIAN", "normalize_affinities": False, "sigma": 0.75}
    return tasks, tcfg, {s: LEVEL_CHANNELS[s] for s in case["strides"]}


def build_head(name, tower_channels=16, fpn=None):
    from range_view_3d_detection_amd.nn.heads.detection_head import DetectionHead

    tasks, tcfg, fpn_default = model_config(name)
    fpn = fpn or fpn_default
    return DetectionHead(fpn=fpn, fpn_kernel_sizes={s: [3, 3] for s in fpn}, targets_config=tcfg, num_classification_blocks=2,
                         num_regression_blocks=2, final_kernel_size=1, tasks_cfg=tasks, task_in_channels=tower_channels, classification_weight=1.0,
                         regression_weight=1.0, coding_weights=[1.0] * 8, classification_head_channels=tower_channels,
                         regression_head_channels=tower_channels, classification_normalization_method="FOREGROUND",
                         _cls_loss={"_target_": "torchbox3d.nn.losses.classification.VarifocalLoss", "alpha": 0.75, "gamma": 2.0, "reduction": "none"},
                         _regression_loss={"_target_": "torch.nn.L1Loss", "reduction": "none"})


# ------------------------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: regenerating the fixtures runs the reference")
def test_generator_reproduces_the_committed_directory(tmp_path):
    """Byte for byte, and not only on the CPU that wrote the files: the generator computes in float64 and stores fp32, so the last-bit
    differences between CPUs (vectorised transcendentals per instruction set, summation order per thread count) do not reach the
    files.  Run twice: as the machine is, and with ATen's scalar code paths on one thread (which moves fp32 results in the last bit)."""
    import subprocess
    import sys

    names = sorted(os.listdir(os.path.join(GOLDEN, "multilevel")))
    assert names == ["A.npz", "B.npz", "C.npz", "D.npz", "common.npz"]
    assert sum(os.path.getsize(os.path.join(GOLDEN, "multilevel", f)) for f in names) < 600 * 1024
    for tag, extra in (("native", {}), ("scalar", {"ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1"})):
        out_dir = tmp_path / tag
        out_dir.mkdir()
        env = dict(os.environ, RV3D_GOLDEN_OUT=str(out_dir), PYTORCH_JIT="0", **extra)
        out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_multilevel.py")], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        for f in names:
            assert open(os.path.join(GOLDEN, "multilevel", f), "rb").read() == open(out_dir / "multilevel" / f, "rb").read(), f"{f} is not reproduced ({tag})"


@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: imports the generator, which imports the reference")
def test_case_table_is_the_generators():
    import subprocess
    import sys

    code = ("import sys, json; sys.path.insert(0, %r); import make_golden_multilevel as m; "
            "print(json.dumps({k: {f: v[f] for f in ('strides', 'classes', 'method', 'partitions')} for k, v in m.CASES.items()}))" % GOLDEN)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTORCH_JIT="0"))
    assert out.returncode == 0, out.stderr[-2000:]
    import json

    theirs = json.loads(out.stdout.strip().splitlines()[-1])
    ours = json.loads(json.dumps(CASES))
    assert theirs == ours


@pytest.mark.parametrize("name", list(CASES))
def test_restated_targets_equal_the_fixture(golden, name):
    g0, g, case = golden("multilevel/common"), golden(f"multilevel/{name}"), CASES[name]
    tg = restate_targets(g0["cart"], g.np("annotations"), case["strides"], case["classes"], case["method"], case["partitions"])
    for s in case["strides"]:
        for t in range(len(case["classes"])):
            for k in ("classification_labels", "panoptics", "points_per_obj"):
                assert torch.equal(tg[s][t][k], g[f"s{s}/t{t}/{k}"]), (name, s, t, k)
            assert torch.allclose(tg[s][t]["regression_targets"], g[f"s{s}/t{t}/regression_targets"], atol=1e-6, rtol=1e-6), (name, s, t)
            n_ref = sum(int((x.unique() > 0).sum()) for x in g[f"s{s}/t{t}/panoptics"])
            assert tg[s][t]["num_objects"] == n_ref


@pytest.mark.parametrize("name", list(CASES))
def test_restated_loss_equals_the_fixture(golden, name):
    g0, g, case = golden("multilevel/common"), golden(f"multilevel/{name}"), CASES[name]
    entries = case_entries(g0, g, name)
    losses, maps = restate_loss(entries, case["strides"])
    ref = unpack(g, "loss")
    assert set(ref) == set(losses)
    for k, v in ref.items():
        assert abs(losses[k] - float(v)) <= 1e-6 * max(1.0, abs(float(v))), (name, k, losses[k], float(v))
    n = len(entries)
    assert float(ref["total_fg"]) == n * float(ref["total_fg/s1"]) and float(ref["total_objects"]) == n * float(ref["total_objects/s1"])
    for e, (soft, fg) in zip(entries, maps):
        assert torch.allclose(soft, g[f"{e['prefix']}/soft"], atol=1e-6) and torch.equal(fg, g[f"{e['prefix']}/foreground"])


def test_fixtures_hold_what_the_cases_are_for(golden):
    """The situations the cases exist for, read from the stored targets (the generator asserts them too, on the reference's run)."""
    g0 = golden("multilevel/common")
    cart = g0["cart"]
    assert cart.shape == (2, 3, 8, 64)
    a, b, c = golden("multilevel/A"), golden("multilevel/B"), golden("multilevel/C")
    assert not (a["annotations"][:, 12] == 1).any() and int(a["s1/t0/panoptics"][1].max()) == 0
    # B: every partition holds an object; the annotation at exactly 15 m owns pixels of level 2 (upper bound inclusive) and none of level 4
    ann = b["annotations"]
    edge = ((ann[:, 0] == 10) & (ann[:, 1] == 11) & (ann[:, 2] == 2)).nonzero().item()
    assert float(ann[edge, :3].norm()) == 15.0
    for s in (1, 2, 4):
        assert int(b[f"s{s}/t0/panoptics"].max()) > 0
    tg = restate_targets(cart, b.np("annotations"), [2, 4], [2], "RANGE", {2: [8.0, 15.0 - 1e-9], 4: [15.0 - 1e-9, INF]})
    assert not torch.equal(tg[2][0]["panoptics"], b["s2/t0/panoptics"]), "the boundary object does not show at level 2"
    # A: an object with pixels at full resolution and none on the columns ::4 (it still consumes a rank there), and ranks that differ
    # between the levels (ranking by the full-resolution counts at every level would show)
    assert a["s4/t0/panoptics"][0].unique().numel() < a["s1/t0/panoptics"][0].unique().numel()
    assert not torch.equal(a["s1/t0/panoptics"][:, :, :, ::4], a["s4/t0/panoptics"]), "the levels rank alike"
    # C: pixels inside boxes of both tasks; task 1 empty in sweep 1
    assert bool(((c["s1/t0/panoptics"] > 0) & (c["s1/t1/panoptics"] > 0)).any())
    assert int(c["s1/t1/panoptics"][1].max()) == 0 and int(c["s1/t1/panoptics"][0].max()) > 0


def test_head_state_dict_keys_for_three_levels_and_two_tasks(golden):
    """Host only: ``classification_head.{stride}.{task}`` / ``regression_head...`` for every level and task, equal to the reference's keys
    (fixture D has strides {1, 2} x two tasks; the key pattern of a third level is checked by construction)."""
    g = golden("multilevel/D")
    head = build_head("D")
    assert {f"head.{k}" for k in head.state_dict()} == set(unpack(g, "sd"))
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {k[len("head."):]: tuple(v.shape) for k, v in unpack(g, "sd").items()}
    from range_view_3d_detection_amd.nn.heads.detection_head import DetectionHead  # noqa: F401

    import test_multilevel_golden as me

    me.CASES["_3x2"] = dict(strides=[1, 2, 4], classes=[3, 2], method=None, partitions={1: [0.0, INF], 2: [0.0, INF], 4: [0.0, INF]})
    try:
        big = build_head("_3x2")
    finally:
        del me.CASES["_3x2"]
    towers = {k.split(".blocks")[0] for k in big.state_dict()}
    assert towers == {f"{kind}.{s}.{t}" for kind in ("classification_head", "regression_head") for s in (1, 2, 4) for t in (0, 1)}
    d_keys = {k.split(".", 3)[3] for k in head.state_dict() if k.startswith("classification_head.1.0.")}
    assert {k.split(".", 3)[3] for k in big.state_dict() if k.startswith("classification_head.1.1.")} == d_keys


def test_points_assignment_still_raises_and_says_why():
    from range_view_3d_detection_amd.nn.heads import detection_head as dh

    with pytest.raises(NotImplementedError, match="overwrites"):
        dh._assignment_method({"fpn_assignment_method": "POINTS"})
    assert dh._assignment_method({"fpn_assignment_method": "RANGE"}) == "RANGE" and dh._assignment_method({"fpn_assignment_method": None}) is None
    assert dh._partition({"range_partitions": {2: [8.0, 15.0]}}, "2") == (8.0, 15.0)


def test_new_entries_are_declared_and_exported():
    from range_view_3d_detection_amd import _lib

    names = ("rv_assign_targets_multilevel", "rv_detection_loss_multilevel_forward", "rv_detection_loss_multilevel_backward", "rv_detection_loss_sums_len")
    assert set(names) <= set(_lib.declared_symbols())
    for tag in ("bf16", "f16"):
        lib = _lib.load(tag)
        assert all(hasattr(lib, n) for n in names)
    assert _lib.loss_sums_len() == 24
