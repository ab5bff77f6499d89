"""Fixtures for the loss KINDS of DetectionHead -- every ``_cls_loss`` / ``_regression_loss`` the configuration can name:
``tests/golden/loss_kinds/{a,b,c,d,e,common}.npz``.

Built like ``make_golden_multilevel.py`` (whose sweep, backbone, annotations and helpers it imports; that module imports
``make_golden``, which installs the stubs and imports the reference): the REFERENCE's own RangeNet + DetectionHead on the CPU, B = 2,
H = 8, W = 64, the same tiny net, everything in float64 on inputs and weights that are exact in fp32, rounded to fp32 once when it is
stored; tower outputs rounded to 1/128 by a forward hook (straight-through gradient), so the directory stays under 600 KiB.  Run by hand
in the build container and by ``tests/test_loss_kinds_golden.py``, which checks that it reproduces the committed directory byte for byte.

* ``a``  PenaltyReducedFocalLoss (alpha 1, gamma 2) + L1Loss, ``normalize_affinities: true``; one level, one task of three classes;
* ``b``  PenaltyReducedFocalLoss (alpha 0.5, gamma 3) + SmoothL1Loss (beta 0.5), ``normalize_affinities: true``; strides {1, 2} x two tasks, RANGE;
* ``c``  FocalLoss configured with alpha 0.6 / gamma 3 + HuberLoss (delta 0.25); one level, one task;
* ``d``  VarifocalLoss + MSELoss; one level, one task;
* ``e``  VarifocalLoss + SmoothL1Loss (beta 0.5); one level, one task.

FocalLoss: the reference's ``forward`` calls ``torchvision.ops.sigmoid_focal_loss(input, target, reduction="none")`` and passes neither
its ``alpha`` nor its ``gamma`` (``nn/losses/classification.py:83``): torchvision's defaults 0.25 / 2 apply, whatever case ``c``
configures.  torchvision is not part of the reference tree and the stub's ``sigmoid_focal_loss`` raises.  This generator does not edit
``_ref_stubs.py``: it BINDS the declared definition (``declared_sigmoid_focal_loss`` below: the published one, as include/rv3d.h states it
for RV_CLS_FOCAL) to the name ``sigmoid_focal_loss`` in ``torchbox3d.nn.losses.classification`` before case ``c`` runs.  What the fixture
pins is therefore the reference's CALL (which arguments reach the function) on top of a definition this project declares.

The generator asserts what the cases are for, on what the reference computed: every PenaltyReducedFocal case has soft targets equal to
1 and soft targets in (0, 1); every SmoothL1 / Huber case has residuals on both sides of the threshold on the pixels that take part;
case ``e``'s loss differs from the loss the same head computes with L1Loss on the same inputs.

Stored per case: annotations, per level the (range-partitioned) mask, per level and task logits / regressands, the four target
tensors, soft targets, foreground, d loss / d logits, d loss / d regressands, and every tensor of the loss dict.  ``common.npz``: the
sweep's ``cart`` and ``mask``.
"""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_multilevel as mm  # noqa: E402  (imports make_golden: installs the stubs and imports the reference)
from make_golden import COLS, DetectionHead, DictConfig, Frame, ListConfig, npy, pack  # noqa: E402

import make_golden as mg  # noqa: E402

OUT_DIR = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "loss_kinds")
INF = math.inf
_CLS = "torchbox3d.nn.losses.classification."

CASES = {
    "a": dict(seed=201, strides=[1], classes=[3], method=None, partitions={1: [0.0, INF]}, normalize=True,
              cls=dict(_target_=_CLS + "PenaltyReducedFocalLoss", alpha=1.0, gamma=2, reduction="none"),
              reg=dict(_target_="torch.nn.L1Loss", reduction="none")),
    "b": dict(seed=212, strides=[1, 2], classes=[2, 1], method="RANGE", partitions={1: [0.0, 10.0], 2: [10.0, INF]}, normalize=True,
              cls=dict(_target_=_CLS + "PenaltyReducedFocalLoss", alpha=0.5, gamma=3, reduction="none"),
              reg=dict(_target_="torch.nn.SmoothL1Loss", reduction="none", beta=0.5)),
    "c": dict(seed=203, strides=[1], classes=[3], method=None, partitions={1: [0.0, INF]}, normalize=False,
              cls=dict(_target_=_CLS + "FocalLoss", alpha=0.6, gamma=3, reduction="none"),
              reg=dict(_target_="torch.nn.HuberLoss", reduction="none", delta=0.25)),
    "d": dict(seed=204, strides=[1], classes=[3], method=None, partitions={1: [0.0, INF]}, normalize=False,
              cls=dict(_target_=_CLS + "VarifocalLoss", alpha=0.75, gamma=2.0, reduction="none"),
              reg=dict(_target_="torch.nn.MSELoss", reduction="none")),
    "e": dict(seed=205, strides=[1], classes=[3], method=None, partitions={1: [0.0, INF]}, normalize=False,
              cls=dict(_target_=_CLS + "VarifocalLoss", alpha=0.75, gamma=2.0, reduction="none"),
              reg=dict(_target_="torch.nn.SmoothL1Loss", reduction="none", beta=0.5)),
}


def declared_sigmoid_focal_loss(inputs, targets, alpha: float = 0.25, gamma: float = 2, reduction: str = "none"):
    """The published sigmoid focal loss with soft targets (include/rv3d.h, RV_CLS_FOCAL): ``alpha_t q^gamma bce``,
    ``q = p (1 - t) + (1 - p) t``, ``alpha_t = alpha t + (1 - alpha)(1 - t)``, no ``alpha_t`` for ``alpha < 0``."""
    p = torch.sigmoid(inputs)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    loss = bce * (p * (1 - targets) + (1 - p) * targets) ** gamma
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    assert reduction == "none"
    return loss


def bind_focal() -> None:
    import torchbox3d.nn.losses.classification as ref_cls

    ref_cls.sigmoid_focal_loss = declared_sigmoid_focal_loss


def same_dtype(module: torch.nn.Module) -> None:
    """The float64 run feeds the regression loss fp64 regressands and the fp32 targets ``compute_targets`` returns; torch's HuberLoss
    refuses that pair in backward.  The target is cast to the input's dtype INSIDE the loss module (exact: every fp32 number is an fp64
    number), for every case alike; nothing else sees the cast (the soft targets keep the dtype the reference gives them)."""
    base = type(module)

    class SameDtype(base):
        def forward(self, input, target):
            return super().forward(input, target.to(input.dtype))

    module.__class__ = SameDtype


class SameDtypeTargets:
    """The reference's soft targets are fp32 tensors even in the float64 run (``assignment.py:116``: ``zeros_like`` of the fp32 regression
    targets), so ``(1 - target).pow(4.0)`` of PenaltyReducedFocalLoss would be an fp32 ``pow``, whose last bit depends on the CPU's
    instruction set -- and with it a stored gradient now and then.  The targets are cast to the logits' dtype on their way INTO the
    classification loss (exact: the same fp32 numbers), for every case alike: the loss is the float64 function of the fp32 soft targets."""

    def __init__(self, loss) -> None:
        self.loss = loss

    def __call__(self, input, target):
        return self.loss(input, target.to(input.dtype))


def build_head(case, tasks):
    level_channels = {1: 2 * mm.WIDTHS[0], 2: mm.WIDTHS[1], 4: mm.WIDTHS[2]}
    tcfg = DictConfig(
        dataset_name="av2", tasks=tasks, enable_azimuth_invariant_targets=True,
        range_partitions=DictConfig({s: case["partitions"][s] for s in case["strides"]}), fpn_assignment_method=case["method"], k=INF,
        affinity_fn="GAUSSIAN", normalize_affinities=case["normalize"], sigma=0.75,
    )
    return DetectionHead(
        fpn=DictConfig({s: level_channels[s] for s in case["strides"]}), fpn_kernel_sizes=DictConfig({s: ListConfig([3, 3]) for s in case["strides"]}),
        targets_config=tcfg, num_classification_blocks=2, num_regression_blocks=2, final_kernel_size=1, tasks_cfg=tasks, task_in_channels=mm.HEAD,
        classification_weight=1.0, regression_weight=1.0, coding_weights=ListConfig([1.0] * 8), classification_head_channels=mm.HEAD,
        regression_head_channels=mm.HEAD, classification_normalization_method="FOREGROUND",
        _cls_loss=DictConfig(**case["cls"]), _regression_loss=DictConfig(**case["reg"]),
    )


def write(name: str, out: dict) -> None:
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    arrays = {k: npy(v) for k, v in out.items()}
    arrays = {k: (a.astype(np.float32) if a.dtype == np.float64 and k != "annotations" else a) for k, a in arrays.items()}
    np.savez_compressed(path, **arrays)
    print(f"loss_kinds/{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


def gen_common() -> None:
    _, _, _, (_, cart, mask) = mm.common(dict(CASES["a"], empty_sweep=None, empty_task=None))
    write("common", {"cart": cart, "mask": mask})


def check_case(name, case, outputs, data, losses, head) -> None:
    """The properties the case exists for, on what the reference computed."""
    strides, n_tasks = case["strides"], len(case["classes"])
    assert float(losses["total_objects"]) >= len(strides) * n_tasks
    kind = case["cls"]["_target_"].rsplit(".", 1)[1]
    reg = case["reg"]["_target_"].rsplit(".", 1)[1]
    for s in strides:
        for t in range(n_tasks):
            assert int(data[s][t]["panoptics"].max()) > 0, (name, s, t, "a (level, task) without any object")
    ones = between = inside = outside = 0
    thr = case["reg"].get("beta", case["reg"].get("delta"))
    for s in strides:
        for t in range(n_tasks):
            soft = data[s][t]["targets"].float()
            ones += int((soft == 1).sum())
            between += int(((soft > 0) & (soft < 1)).sum())
            on = (data[s][t]["classification_labels"] < case["classes"][t])[:, None] & outputs[s]["mask"].bool()
            d = (outputs[s][t]["regressands"].detach() - data[s][t]["regression_targets"]).abs()
            if thr is not None:
                inside += int(((d < thr) & on).sum())
                outside += int(((d > thr) & on).sum())
    if kind == "PenaltyReducedFocalLoss":
        assert ones >= 1 and between >= 1, (name, ones, between)
    if thr is not None:
        assert inside >= 1 and outside >= 1, (name, inside, outside)
    if name == "e":
        head.regression_loss = torch.nn.L1Loss(reduction="none")
        same_dtype(head.regression_loss)
        with torch.no_grad():
            l1 = head.loss(outputs, data)
        assert abs(float(l1["regression_loss"]) - float(losses["regression_loss"])) > 1e-3 * float(losses["regression_loss"]), "SmoothL1 reads as L1"
    print(f"loss_kinds/{name}: {kind} + {reg}: t == 1: {ones}, 0 < t < 1: {between}, |d| < thr: {inside}, > thr: {outside}")


def gen_case(name: str) -> None:
    case = dict(CASES[name], empty_sweep=None, empty_task=None)
    backbone, _, tasks, (features, cart, mask) = mm.common(case)
    head = build_head(case, tasks)
    if case["cls"]["_target_"].endswith(".FocalLoss"):
        bind_focal()
    g = torch.Generator().manual_seed(case["seed"])
    torch.manual_seed(case["seed"])
    mg.randomize_bn(head, g)
    mg._open_gates(head)
    for pname, p in head.named_parameters():
        if pname.endswith("0.weight"):
            p.data = 0.08 * torch.randn(p.shape, generator=g)
    for s in case["strides"]:
        for t in range(len(case["classes"])):
            head.classification_head[str(s)][str(t)].blocks[-1][0].bias.data.fill_(-1.0)
            head.classification_head[str(s)][str(t)].register_forward_hook(mm._round_outputs)
            head.regression_head[str(s)][str(t)].register_forward_hook(mm._round_outputs)
    mg._coarse(head)
    head.double()
    same_dtype(head.regression_loss)
    head.cls_loss = SameDtypeTargets(head.cls_loss)
    ann = mm.annotations(g, cart, mask, case["classes"], None, None)
    frame = Frame({c: ann[:, i] for i, c in enumerate(COLS)})
    out: dict = {"annotations": ann}
    backbone.train()
    head.train()
    data = {"features": features.double(), "cart": cart.double(), "mask": mask, "annotations": frame}
    feats = backbone(data)
    outputs, losses = head(feats, data, return_loss=True)
    for s in case["strides"]:
        for t in range(len(case["classes"])):
            outputs[s][t]["logits"].retain_grad()
            outputs[s][t]["regressands"].retain_grad()
    losses["loss"].backward()
    for s in case["strides"]:
        out[f"s{s}/mask"] = outputs[s]["mask"]
        for t in range(len(case["classes"])):
            p = f"s{s}/t{t}"
            out[f"{p}/logits"], out[f"{p}/regressands"] = outputs[s][t]["logits"], outputs[s][t]["regressands"]
            out[f"{p}/d_logits"], out[f"{p}/d_regressands"] = outputs[s][t]["logits"].grad, outputs[s][t]["regressands"].grad
            for k in ("classification_labels", "panoptics", "regression_targets", "points_per_obj"):
                out[f"{p}/{k}"] = data[s][t][k]
            out[f"{p}/soft"] = data[s][t]["targets"]
            out[f"{p}/foreground"] = losses["aux"][s][t]["foreground"]
    pack(out, "loss", {k: v.detach().float().reshape(1) for k, v in losses.items() if isinstance(v, torch.Tensor)})
    check_case(name, case, outputs, data, losses, head)
    write(name, out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case_name in sys.argv[1:] or ["common"] + list(CASES):
        gen_common() if case_name == "common" else gen_case(case_name)
