"""Fixtures for soft target assignment with every option of ``targets_config``: ``tests/golden/assignment/{A..F}.npz``.

Runs the REFERENCE's own ``compute_targets``, ``compute_classification_targets`` (``math/ops/assignment.py:76-147``) and
``DetectionHead.forward(..., return_loss=True)`` / ``backward()`` on the CPU, on the sweep of ``multilevel/common.npz``.  The towers are
not part of this: every tower's ``forward`` is bound to a tensor made here (logits and regressands on a 1/128 grid), so everything the
fixtures hold -- the RANGE mask, targets, per-instance affinities, top-k selection, loss dict, gradients -- is what the reference computes
from those tensors.  Regressands are the reference's regression targets plus noise, so that affinities spread over (0, 1].

For the BEV cases ``mmcv.ops.box_iou_rotated`` (absent here) is bound to a stand-in with mmcv's signature over
``oracle.nms.pairwise_iou`` -- the tree's declared rotated-IoU geometry, ``(cx, cy, w, h, angle) -> [x1, y1, x2, y2, ry]``, the diagonal
for ``aligned=True`` -- exactly as ``make_golden.py`` binds ``wnms_gpu``: the wrapper logic (column choice, ``.float()``, clamp, top-k,
scatter) is the reference's.  The IoU of one pair does not change when both angles change sign, so mmcv's angle convention does not enter.

* ``A``  GAUSSIAN, ``k = 4``: instances with fewer than 4 pixels, exactly 4 and many more; sweep 1 has no annotation; one pixel with
         ``mask == 0`` (valid geometry, flagged invalid) lies inside an instance's set and inside its top 4;
* ``B``  GAUSSIAN, ``normalize_affinities``, ``k = inf``: every instance has a pixel with affinity exactly 1;
* ``C``  GAUSSIAN, normalised, ``k = 16``;
* ``D``  BEV, ``k = inf``: instances in which some pixels have IoU 0 (foreground count < set size) and one whose pixels all do;
* ``E``  BEV, ``k = 8``;
* ``F``  strides {1, 2} x two tasks, RANGE, GAUSSIAN ``k = 4``: the selection is per (level, task, sweep, instance).
The generator asserts these situations, and that in every instance the k-th and (k+1)-th largest affinities differ by more than 1e-4
relative: no fixture depends on the tie rule or on the last bit of an exponential.

Reproducible byte for byte on any CPU, like ``make_golden_multilevel.py``: float64 compute on inputs that are exact in fp32, fp32 stored.
"""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stubs and imports the reference)
import make_golden_multilevel as mm  # noqa: E402  (its annotation sampler)
from make_golden import COLS, DetectionHead, DictConfig, Frame, ListConfig, npy, pack  # noqa: E402

from torchbox3d.math.ops import assignment as ref_assignment  # noqa: E402
from torchbox3d.nn.heads.detection_head import compute_targets as ref_compute_targets  # noqa: E402

OUT_DIR = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "assignment")
INF = math.inf
FAR = 40.0  # metres added to a prediction's x offset: its BEV rectangle is disjoint from the target's

CASES = {
    "A": dict(seed=227, strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="GAUSSIAN", normalize=False, k=4, empty_sweep=1),
    "B": dict(seed=202, strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="GAUSSIAN", normalize=True, k=INF, empty_sweep=None),
    "C": dict(seed=203, strides=[1], classes=[3], method=None, partitions={1: [0.0, INF]}, affinity_fn="GAUSSIAN", normalize=True, k=16, empty_sweep=None),
    "D": dict(seed=204, strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="BEV", normalize=False, k=INF, empty_sweep=None),
    "E": dict(seed=205, strides=[1], classes=[2], method=None, partitions={1: [0.0, INF]}, affinity_fn="BEV", normalize=False, k=8, empty_sweep=None),
    "F": dict(seed=208, strides=[1, 2], classes=[2, 1], method="RANGE", partitions={1: [0.0, 10.0], 2: [10.0, INF]}, affinity_fn="GAUSSIAN",
              normalize=False, k=4, empty_sweep=None),
}


def box_iou_rotated(bboxes1, bboxes2, mode="iou", aligned=False, clockwise=True):
    """``mmcv.ops.box_iou_rotated`` over ``oracle.nms.pairwise_iou``: boxes ``(cx, cy, w, h, angle)``, fp32."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import nms as onms

    assert mode == "iou" and bboxes1.dtype == torch.float32 and bboxes2.dtype == torch.float32

    def corners(b):
        b = b.detach().numpy().astype(np.float32)
        hw, hh = np.float32(0.5) * b[:, 2], np.float32(0.5) * b[:, 3]
        return np.stack([b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh, b[:, 4]], axis=1)

    iou = torch.from_numpy(onms.pairwise_iou(corners(bboxes1), corners(bboxes2)))
    return iou.diagonal().clone() if aligned else iou


def targets_config(case, tasks, k=None):
    return DictConfig(
        dataset_name="av2", tasks=tasks, enable_azimuth_invariant_targets=True,
        range_partitions=DictConfig({s: case["partitions"][s] for s in case["strides"]}), fpn_assignment_method=case["method"],
        k=case["k"] if k is None else k, affinity_fn=case["affinity_fn"], normalize_affinities=case["normalize"], sigma=0.75,
    )


def build_head(case, tasks, tcfg):
    head = DetectionHead(
        fpn=DictConfig({s: 8 for s in case["strides"]}), fpn_kernel_sizes=DictConfig({s: ListConfig([3, 3]) for s in case["strides"]}),
        targets_config=tcfg, num_classification_blocks=1, num_regression_blocks=1, final_kernel_size=1, tasks_cfg=tasks, task_in_channels=8,
        classification_weight=1.0, regression_weight=1.0, coding_weights=ListConfig([1.0] * 8), classification_head_channels=8,
        regression_head_channels=8, classification_normalization_method="FOREGROUND",
        _cls_loss=DictConfig(_target_="torchbox3d.nn.losses.classification.VarifocalLoss", alpha=0.75, gamma=2.0, reduction="none"),
        _regression_loss=DictConfig(_target_="torch.nn.L1Loss", reduction="none"),
    )
    return head.double().train()


def grid(t):
    return torch.round(t * 128) / 128


def instances(pan):
    """(sweep, id, flat pixel indices) of every instance of a panoptic map (B,1,H,W)."""
    for b in range(pan.shape[0]):
        flat = pan[b].reshape(-1)
        for p in flat.unique().tolist():
            if p > 0:
                yield b, p, (flat == p).nonzero().flatten()


def gen_case(name: str) -> None:
    case = CASES[name]
    common = np.load(os.path.join(HERE, "multilevel", "common.npz"))
    cart, mask = torch.from_numpy(common["cart"]), torch.from_numpy(common["mask"]).clone()
    B, _, H, W = cart.shape
    g = torch.Generator().manual_seed(case["seed"])
    torch.manual_seed(case["seed"])
    ann = mm.annotations(g, cart, mask, case["classes"], case["empty_sweep"], None)
    frame = Frame({c: ann[:, i] for i, c in enumerate(COLS)})
    tasks = DictConfig({t: ListConfig([f"T{t}C{i}" for i in range(n)]) for t, n in enumerate(case["classes"])})
    tcfg = targets_config(case, tasks)
    ref_assignment.box_iou_rotated = box_iou_rotated
    cart64 = cart.double()

    # pass one: the reference's targets, to put the regressands near them
    tg0 = ref_compute_targets({"cart": cart64, "annotations": frame}, tasks_config=tasks, fpn_strides=case["strides"], targets_config=tcfg)
    masked_pixel = None
    if name == "A":  # a pixel of valid geometry flagged invalid, inside a large instance of sweep 0
        pan = tg0[1][0]["panoptics"]
        b, p, idx = max(((b, p, idx) for b, p, idx in instances(pan) if b == 0), key=lambda x: x[2].numel())
        masked_pixel = (b, int(idx[idx.numel() // 2]))
        assert bool(mask.view(B, -1)[masked_pixel]) and idx.numel() > 4
        mask.view(B, -1)[masked_pixel] = False
    leaves, all_zero = {}, None
    for s in case["strides"]:
        for t, n_cls in enumerate(case["classes"]):
            ws = W // s
            reg_t = tg0[s][t]["regression_targets"].double()
            noise = (torch.rand(B, 8, H, ws, generator=g).double() * 2 - 1) * torch.tensor([0.6, 0.6, 0.6, 0.2, 0.2, 0.2, 0.2, 0.2]).double().view(1, 8, 1, 1)
            reg = reg_t + noise
            pan = tg0[s][t]["panoptics"]
            if case["affinity_fn"] == "BEV":
                insts = list(instances(pan))
                all_zero = max(insts, key=lambda x: x[2].numel() if 3 <= x[2].numel() <= 12 else 0)[:2]
                for b, p, idx in insts:
                    far = idx if (b, p) == all_zero else idx[torch.rand(idx.numel(), generator=g) < 0.2]
                    reg[b, 0].view(-1)[far] += FAR
            if masked_pixel is not None:
                reg[masked_pixel[0]].view(8, -1)[:, masked_pixel[1]] = reg_t[masked_pixel[0]].view(8, -1)[:, masked_pixel[1]]
            leaves[(s, t)] = (grid(torch.randn(B, n_cls, H, ws, generator=g).double() - 1.0).requires_grad_(True), grid(reg).requires_grad_(True))

    # pass two: the reference's forward with every tower bound to its tensor
    head = build_head(case, tasks, tcfg)
    for (s, t), (logits, reg) in leaves.items():
        head.classification_head[str(s)][str(t)].forward = lambda *a, _v=logits: _v
        head.regression_head[str(s)][str(t)].forward = lambda *a, _v=reg: _v
    data = {"features": torch.zeros(B, 1, H, W, dtype=torch.float64), "cart": cart64, "mask": mask, "annotations": frame}
    outputs, losses = head({s: None for s in case["strides"]}, data, return_loss=True)
    losses["loss"].backward()

    out: dict = {"annotations": ann, "mask": mask}
    seen = {"small": False, "exact": False, "large": False, "partial_zero": False, "all_zero": False, "one": True, "masked_top": False}
    tcfg_all = targets_config(case, tasks, k=INF)
    for s in case["strides"]:
        out[f"s{s}/mask"] = outputs[s]["mask"]
        for t, n_cls in enumerate(case["classes"]):
            p = f"s{s}/t{t}"
            logits, reg = leaves[(s, t)]
            tg = data[s][t]
            fg = losses["aux"][s][t]["foreground"]
            for k_ in ("classification_labels", "panoptics", "regression_targets", "points_per_obj"):
                out[f"{p}/{k_}"] = tg[k_]
                assert torch.equal(tg[k_], tg0[s][t][k_])
            out[f"{p}/logits"], out[f"{p}/regressands"], out[f"{p}/d_logits"], out[f"{p}/d_regressands"] = logits, reg, logits.grad, reg.grad
            out[f"{p}/soft"], out[f"{p}/foreground"] = tg["targets"], fg
            # every affinity before the selection (the reference's function with k = inf), for the checks below
            soft_all, _, _, _ = ref_assignment.compute_classification_targets(
                reg, tg["regression_targets"], tg["classification_labels"], outputs[s]["cart"], tcfg_all, outputs[s]["mask"], tg["panoptics"], n_cls)
            assert int(tg["panoptics"].max()) > 0, (name, s, t, "a (level, task) without any instance")
            aff_all, aff = soft_all.detach().sum(dim=1).view(B, -1), tg["targets"].detach().sum(dim=1).view(B, -1)
            for b, pid, idx in instances(tg["panoptics"]):
                a = aff_all[b, idx].sort(descending=True).values
                n, k = idx.numel(), case["k"]
                kept = int((aff[b, idx] != 0).sum())
                assert kept == int(fg.view(B, -1)[b, idx].sum())
                if k != INF:
                    seen["small"] |= n < k
                    seen["exact"] |= n == k
                    seen["large"] |= n > 2 * k
                    if n > k:
                        assert float(a[k - 1] - a[k]) > 1e-4 * float(a[k - 1]) or float(a[k - 1]) == 0.0, (name, s, t, b, pid, "k-th and (k+1)-th affinity too close")
                        assert kept == int((a[:k] != 0).sum())
                if case["normalize"]:
                    seen["one"] &= float(a[0]) == 1.0
                zeros = int((a == 0).sum())
                seen["partial_zero"] |= 0 < zeros < n
                seen["all_zero"] |= zeros == n
                if masked_pixel is not None and b == masked_pixel[0] and bool((idx == masked_pixel[1]).any()):
                    seen["masked_top"] = float(aff[b, masked_pixel[1]]) != 0.0 and not bool(outputs[s]["mask"].view(B, -1)[b, masked_pixel[1]])
    if case["k"] != INF:
        assert seen["large"] and (name != "A" or (seen["small"] and seen["exact"])), (name, seen)
    if name == "A":
        assert seen["masked_top"] and int(data[1][0]["panoptics"][1].max()) == 0, (name, seen)
    if case["normalize"]:
        assert seen["one"], name
    if name == "D":
        assert seen["partial_zero"] and seen["all_zero"], (name, seen)
    pack(out, "loss", {k_: v.detach().float().reshape(1) for k_, v in losses.items() if isinstance(v, torch.Tensor)})
    write(name, out)


def write(name: str, out: dict) -> None:
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    arrays = {k: npy(v) for k, v in out.items()}
    arrays = {k: (a.astype(np.float32) if a.dtype == np.float64 and k != "annotations" else a) for k, a in arrays.items()}
    np.savez_compressed(path, **arrays)
    print(f"assignment/{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case_name in sys.argv[1:] or list(CASES):
        gen_case(case_name)
