"""Fixtures for DetectionHead with several FPN strides and several tasks: ``tests/golden/multilevel/{A,B,C,D}.npz``.

Like ``make_golden.py`` (whose stub loader and helpers it imports) this runs the REFERENCE's own RangeNet + DetectionHead +
RangeDecoder on the CPU; it is run by hand in the build container and by ``tests/test_multilevel_golden.py``, which checks that it
reproduces the committed directory byte for byte.  Every case: B = 2, H = 8, W = 64, BASIC stem, widths [8, 8, 16, 16, 16], towers of
two blocks and 16 channels, BatchNorm gates open, weights on a 1/64 grid.  The sweep and the backbone's state dict are the same in all
cases and stored once, in ``common.npz``.  To keep the directory under 600 KiB the towers' outputs are rounded to multiples of 1/128 by
a forward hook (straight-through gradient): fp32 noise does not compress, and logits / regressands are most of a case.  Everything
downstream of the towers -- targets, loss, gradients, decode -- is what the reference computes from those rounded outputs.

* ``A``  strides {1, 2, 4}, one task, ``fpn_assignment_method: null``; sweep 1 has no annotation;
* ``B``  strides {1, 2, 4}, one task, RANGE with partitions (0, 8], (8, 15], (15, inf): each holds objects; one centre at exactly 15 m
         (it belongs to the level of stride 2); one object of the far partition with a pixel at full resolution and none on the columns ::4;
* ``C``  stride {1}, two tasks (3 + 2 classes): nested boxes of the same task and of different tasks; task 1 is empty in sweep 1;
* ``D``  strides {1, 2} x two tasks, RANGE with partitions (0, 10], (10, inf).
The generator asserts these properties on what the reference computed, so a change of seed cannot silently lose them.

Reproducible on any machine, not only on the one that wrote the files: fp32 results of the same torch build differ in the last bit
between CPUs (vectorised exp / sin / cos per instruction set, summation order per thread count), so the whole run -- sweep,
backbone, head, targets, loss, backward, decode -- is done in float64 on inputs and weights that are exact in fp32, and rounded to
fp32 once, when it is stored: noise of 1e-16 does not move an fp32 rounding.  The reference's own fp32 steps (box vertices, centre
offsets cast with ``.float()``) stay as they are; what it would compute in fp32 from fp32 inputs lies within fp32 rounding of the
stored values, which is what the tests' tolerances (1e-6 and up) allow for.

Stored per case: inputs, annotations, state dict (packed), per level the masked ``mask``, per level and task logits / regressands, all
target tensors, soft targets, foreground, every tensor of the loss dict, d loss / d logits and d loss / d regressands element by
element, parameter-gradient summaries (``grad_summary``), and ``decode(..., use_nms=False)`` of the eval-mode model.
"""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)
from make_golden import COLS, DetectionHead, DictConfig, Frame, ListConfig, RangeDecoder, RangeNet, grad_summary, npy, pack  # noqa: E402

OUT_DIR = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "multilevel")
B, H, W = 2, 8, 64
WIDTHS = [8, 8, 16, 16, 16]
HEAD = 16
BLOCK_RANGES = [5.0, 7.0, 11.0, 15.0, 20.0, 13.0, 6.0, 18.0, 5.0]  # range of the columns (w + 4) // 8: near, middle and far partitions

CASES = {
    "A": dict(seed=101, strides=[1, 2, 4], classes=[2], method=None, partitions={1: [0.0, math.inf], 2: [0.0, math.inf], 4: [0.0, math.inf]},
              empty_sweep=1, empty_task=None),
    "B": dict(seed=102, strides=[1, 2, 4], classes=[2], method="RANGE", partitions={1: [0.0, 8.0], 2: [8.0, 15.0], 4: [15.0, math.inf]},
              empty_sweep=None, empty_task=None),
    "C": dict(seed=103, strides=[1], classes=[3, 2], method=None, partitions={1: [0.0, math.inf]}, empty_sweep=None, empty_task=(1, 1)),
    "D": dict(seed=104, strides=[1, 2], classes=[2, 1], method="RANGE", partitions={1: [0.0, 10.0], 2: [10.0, math.inf]},
              empty_sweep=None, empty_task=None),
}


def sweep(g: torch.Generator):
    """Range image whose columns come in blocks of eight at the ranges of BLOCK_RANGES (+ a little relief), so that every range
    partition holds surfaces to put boxes on."""
    az = torch.linspace(math.pi, -math.pi, W, dtype=torch.float64).view(1, 1, 1, W)
    inc = torch.linspace(0.2, -0.4, H, dtype=torch.float64).view(1, 1, H, 1)
    base = torch.tensor([BLOCK_RANGES[(w + 4) // 8] for w in range(W)], dtype=torch.float64).view(1, 1, 1, W)
    r = base + 0.3 * torch.cos(7 * inc) + 0.2 * torch.rand(B, 1, H, W, generator=g).double()
    mask = torch.rand(B, 1, H, W, generator=g) >= 0.08
    cart = torch.cat([r * inc.cos() * az.cos(), r * inc.cos() * az.sin(), r * inc.sin().expand(B, 1, H, W)], dim=1) * mask
    features = torch.cat([torch.rand(B, 1, H, W, generator=g).double(), r, cart], dim=1) * mask
    return features.float(), cart.float(), mask  # (fp64 trigonometry rounded once: the same fp32 numbers on every CPU)


def annotations(g: torch.Generator, cart: torch.Tensor, mask: torch.Tensor, classes, empty_sweep, empty_task) -> np.ndarray:
    """(M,13) fp64 rows [xyz, lwh, qwxyz, task, offset, batch] sorted by (sweep, task): boxes on valid pixels, every third one a large
    box around its predecessor (alternately of the same and of another task), plus the two special objects of sweep 0."""
    rows = []
    n_tasks = len(classes)
    for b in range(B):
        if b == empty_sweep:
            continue
        valid = mask[b, 0].nonzero()
        pick = valid[torch.randperm(valid.shape[0], generator=g)[:9]]
        sweep_rows = []
        for i, (h, w) in enumerate(pick.tolist()):
            ctr = cart[b, :, h, w].double()
            lwh = torch.tensor([1.0, 1.0, 1.0]) + torch.rand(3, generator=g) * torch.tensor([4.0, 2.0, 2.0])
            task = i % n_tasks
            if i % 3 == 1:
                ctr = torch.tensor(sweep_rows[-1][:3])
                lwh = torch.tensor(sweep_rows[-1][3:6]) * 2.5
                task = int(sweep_rows[-1][10]) if (i // 3) % 2 == 0 else (int(sweep_rows[-1][10]) + 1) % n_tasks
            yaw = (torch.rand(1, generator=g).item() * 2 - 1) * math.pi
            cat = int(torch.randint(0, classes[task], (1,), generator=g).item())
            sweep_rows.append(ctr.tolist() + lwh.double().tolist() + [math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)] + [float(task), float(cat), float(b)])
        if b == 0:
            # centre at exactly 15 m (10^2 + 11^2 + 2^2 = 225) on the block of columns at that range
            sweep_rows.append([10.0, 11.0, 2.0, 4.0, 3.0, 3.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
            # one pixel of the far block on a column = 1 (mod 4): a unit box there holds that pixel only
            hw = [(h, w) for h, w in valid.tolist() if w in (29, 33)][0]
            sweep_rows.append(cart[b, :, hw[0], hw[1]].double().tolist() + [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, float(classes[0] - 1), 0.0])
        if empty_task is not None and empty_task[0] == b:
            sweep_rows = [r for r in sweep_rows if int(r[10]) != empty_task[1]]
        sweep_rows.sort(key=lambda r: r[10])  # stable: by task, original order within a task
        rows += sweep_rows
    return np.asarray(rows, dtype=np.float64)


def build(case):
    L = ListConfig(WIDTHS)
    backbone = RangeNet(
        in_channels=5, layers=L, out_channels=WIDTHS[0], projection_kernel_size=1, dataset_name="av2", num_neighbors=3, num_layers=2,
        stem_type="BASIC", _net=DictConfig(_target_="torchbox3d.nn.backbones.dla.RangeBackbone", in_channels=5, layers=L, out_channels=WIDTHS[0]),
    )
    level_channels = {1: 2 * WIDTHS[0], 2: WIDTHS[1], 4: WIDTHS[2]}  # as RangeNet returns them
    tasks = DictConfig({t: ListConfig([f"T{t}C{i}" for i in range(n)]) for t, n in enumerate(case["classes"])})
    tcfg = DictConfig(
        dataset_name="av2", tasks=tasks, enable_azimuth_invariant_targets=True,
        range_partitions=DictConfig({s: case["partitions"][s] for s in case["strides"]}), fpn_assignment_method=case["method"], k=math.inf,
        affinity_fn="GAUSSIAN", normalize_affinities=False, sigma=0.75,
    )
    head = DetectionHead(
        fpn=DictConfig({s: level_channels[s] for s in case["strides"]}), fpn_kernel_sizes=DictConfig({s: ListConfig([3, 3]) for s in case["strides"]}),
        targets_config=tcfg, num_classification_blocks=2, num_regression_blocks=2, final_kernel_size=1, tasks_cfg=tasks, task_in_channels=HEAD,
        classification_weight=1.0, regression_weight=1.0, coding_weights=ListConfig([1.0] * 8), classification_head_channels=HEAD,
        regression_head_channels=HEAD, classification_normalization_method="FOREGROUND",
        _cls_loss=DictConfig(_target_="torchbox3d.nn.losses.classification.VarifocalLoss", alpha=0.75, gamma=2.0, reduction="none"),
        _regression_loss=DictConfig(_target_="torch.nn.L1Loss", reduction="none"),
    )
    return backbone, head, tasks


def check_case(name, case, ann, data, losses):
    """The properties the case exists for, on what the reference computed."""
    strides = case["strides"]
    n_entries = len(strides) * len(case["classes"])
    assert float(losses["total_objects"]) >= n_entries, "every case needs objects"
    for s in strides:
        for t in range(len(case["classes"])):
            assert int(data[s][t]["panoptics"].max()) > 0 or (name == "C"), (name, s, t, "a (level, task) without any object")
    if case["empty_sweep"] is not None:
        assert not (ann[:, 12] == case["empty_sweep"]).any()
        assert int(data[1][0]["panoptics"][case["empty_sweep"]].max()) == 0
    if name in ("A", "B"):
        far = ann[(ann[:, 12] == 0) & (ann[:, 3] == 1.0) & (ann[:, 4] == 1.0) & (ann[:, 5] == 1.0)][0]
        assert np.linalg.norm(far[:3]) > 15.0  # the unit box on one pixel of the far block, on a column = 1 (mod 4)
        assert data[4][0]["panoptics"][0].unique().numel() < data[1][0]["panoptics"][0].unique().numel() or name == "B"
        on_edge = ann[(ann[:, 0] == 10.0) & (ann[:, 1] == 11.0)]
        assert on_edge.shape[0] == 1 and np.linalg.norm(on_edge[0, :3]) == 15.0
    if name == "C":
        assert not ((ann[:, 12] == 1) & (ann[:, 10] == 1)).any() and ((ann[:, 12] == 0) & (ann[:, 10] == 1)).any()
        both = (data[1][0]["panoptics"] > 0) & (data[1][1]["panoptics"] > 0)
        assert bool(both.any()), "no pixel inside boxes of both tasks"


COMMON_SEED = 100


def common(case):
    """The sweep and the backbone every case shares (own seed), and the case's head."""
    g = torch.Generator().manual_seed(COMMON_SEED)
    torch.manual_seed(COMMON_SEED)
    backbone, head, tasks = build(case)
    mg.randomize_bn(backbone, g)
    mg._open_gates(backbone)
    mg._coarse(backbone)
    return backbone.double(), head, tasks, sweep(g)


def _round_outputs(module, inputs, output):
    return output + (torch.round(output * 128) / 128 - output).detach()


def gen_common() -> None:
    backbone, _, _, (features, cart, mask) = common(CASES["A"])
    out: dict = {"features": features, "cart": cart, "mask": mask}
    pack(out, "sd", {f"backbone.{k}": v.clone() for k, v in backbone.state_dict().items()})
    write("common", out)


def write(name: str, out: dict) -> None:
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    arrays = {k: npy(v) for k, v in out.items()}
    arrays = {k: (a.astype(np.float32) if a.dtype == np.float64 and k != "annotations" else a) for k, a in arrays.items()}
    np.savez_compressed(path, **arrays)
    print(f"multilevel/{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


def gen_case(name: str) -> None:
    case = CASES[name]
    backbone, head, tasks, (features, cart, mask) = common(case)
    g = torch.Generator().manual_seed(case["seed"])
    torch.manual_seed(case["seed"])
    mg.randomize_bn(head, g)
    mg._open_gates(head)
    for pname, p in head.named_parameters():
        if pname.endswith("0.weight"):
            p.data = 0.08 * torch.randn(p.shape, generator=g)
    for s in case["strides"]:
        for t in range(len(case["classes"])):
            head.classification_head[str(s)][str(t)].blocks[-1][0].bias.data.fill_(-1.0)  # so that some scores pass 0.1
            head.classification_head[str(s)][str(t)].register_forward_hook(_round_outputs)
            head.regression_head[str(s)][str(t)].register_forward_hook(_round_outputs)
    mg._coarse(head)
    head.double()
    ann = annotations(g, cart, mask, case["classes"], case["empty_sweep"], case["empty_task"])
    frame = Frame({c: ann[:, i] for i, c in enumerate(COLS)})

    out: dict = {"annotations": ann}
    sd0 = {**{f"backbone.{k}": v.clone() for k, v in backbone.state_dict().items()}, **{f"head.{k}": v.clone() for k, v in head.state_dict().items()}}
    pack(out, "sd", {k: v for k, v in sd0.items() if k.startswith("head.")})  # (the backbone's is in common.npz)

    backbone.train()
    head.train()
    features64, cart64 = features.double(), cart.double()  # (the stored fp32 numbers, exactly)
    data = {"features": features64, "cart": cart64, "mask": mask, "annotations": frame}
    feats = backbone(data)
    outputs, losses = head(feats, data, return_loss=True)
    for s in case["strides"]:
        for t in range(len(case["classes"])):
            outputs[s][t]["logits"].retain_grad()
            outputs[s][t]["regressands"].retain_grad()
    losses["loss"].backward()
    check_case(name, case, ann, data, losses)
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
    grads = {**{f"backbone.{k}": p.grad for k, p in backbone.named_parameters()}, **{f"head.{k}": p.grad for k, p in head.named_parameters()}}
    pack(out, "grad_summary", {k: grad_summary(k, v) for k, v in grads.items()})

    backbone.load_state_dict({k[len("backbone."):]: v for k, v in sd0.items() if k.startswith("backbone.")})
    head.load_state_dict({k[len("head."):]: v for k, v in sd0.items() if k.startswith("head.")})
    backbone.eval()
    head.eval()
    with torch.no_grad():
        data = {"features": features64, "cart": cart64, "mask": mask}
        outputs, _ = head(backbone(data), data, return_loss=False)
        dec = RangeDecoder(True, True, ListConfig([0, 15, 30]), ListConfig([15, 30, math.inf]), ListConfig([8, 2, 1]))
        params, scores, cats, bidx = dec.decode(
            outputs, DictConfig(num_pre_nms=50000, num_post_nms=1000, nms_threshold=0.3, min_confidence=0.1, nms_mode="WEIGHTED"), tasks, use_nms=False)
        out["eval/dec_params"], out["eval/dec_scores"], out["eval/dec_categories"], out["eval/dec_batch_index"] = params, scores, cats, bidx
        if len(case["classes"]) > 1:
            assert int(cats.max()) >= case["classes"][0], "no detection of the second task: its category offset would go unseen"
    write(name, out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case_name in sys.argv[1:] or ["common"] + list(CASES):
        gen_common() if case_name == "common" else gen_case(case_name)
