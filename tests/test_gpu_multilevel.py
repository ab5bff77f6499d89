"""DetectionHead with several FPN strides and several tasks on the device: ``rv_assign_targets_multilevel``, the two-phase loss
(``rv_detection_loss_multilevel_forward`` / ``_backward``), the head that calls them, and the decoder's first run on more than one level.

Yardsticks: the fixtures of ``tests/golden/multilevel/`` (the reference itself on the CPU) and, at full size, the plain-torch
restatement of tests/test_multilevel_golden.py (pinned to those fixtures there).  Outputs a kernel must write completely are
pre-filled with NaN / a sentinel.
"""

from __future__ import annotations

import ctypes
import math

import pytest
import torch

from test_gpu_backward import _cos
from test_gpu_forward import DEV, rel_err
from test_multilevel_golden import CASES, INF, build_head, case_entries, restate_loss, restate_targets
from test_oracle_golden import grad_summary, unpack

pytestmark = pytest.mark.gpu

SENTINEL = -12345
HP = {"coding_weights": [1.0] * 8, "cls_weight": 1.0, "reg_weight": 1.0, "smoothing": 1.0, "sigma": 0.75, "alpha": 0.75, "gamma": 2.0, "az_inv": True}


def _targets_through_the_c_abi(cart, annotations, case):
    """rv_assign_targets_multilevel on sentinel-filled outputs -> ({stride: {task: targets}}, num_objects (levels * tasks) on the CPU)."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.nn.heads import detection_head as dh

    B, _, H, W = cart.shape
    strides, classes = case["strides"], case["classes"]
    cub_d, off_d, m = dh._stage_annotations({"annotations": annotations}, B, DEV)
    cart32 = cart.to(DEV).float().contiguous()
    n_l, n_t = len(strides), len(classes)
    levels = (L.TargetLevel * n_l)(*[L.TargetLevel(s, 1 if case["method"] == "RANGE" else 0, *[float(v) for v in case["partitions"][s]]) for s in strides])
    outs = (L.TargetOut * (n_l * n_t))()
    res = {}
    for i, s in enumerate(strides):
        res[s] = {}
        for t in range(n_t):
            ws = W // s
            tg = {"classification_labels": torch.full((B, H, ws), SENTINEL, dtype=torch.int64, device=DEV),
                  "panoptics": torch.full((B, 1, H, ws), SENTINEL, dtype=torch.int64, device=DEV),
                  "regression_targets": torch.full((B, 8, H, ws), float("nan"), device=DEV),
                  "points_per_obj": torch.full((B, 1, H, ws), SENTINEL, dtype=torch.int64, device=DEV)}
            outs[i * n_t + t] = L.TargetOut(tg["classification_labels"].data_ptr(), tg["panoptics"].data_ptr(), tg["regression_targets"].data_ptr(),
                                            tg["points_per_obj"].data_ptr())
            res[s][t] = tg
    nobj = torch.full((n_l * n_t,), SENTINEL, dtype=torch.int32, device=DEV)
    scratch = torch.full((3 * n_l * max(m, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    L.call("rv_assign_targets_multilevel", L.ptr(cub_d) if m else None, m, L.ptr(off_d), L.ptr(cart32), B, H, W, n_l,
           levels, n_t, (ctypes.c_int32 * n_t)(*range(n_t)), (ctypes.c_int32 * n_t)(*classes), 1, L.ptr(scratch), outs, L.ptr(nobj),
           L.stream_ptr())
    torch.cuda.synchronize()
    return res, nobj.cpu()


def _assert_targets(got, nobj, ref, case, tag):
    """``ref``: {stride: {task: targets}} with integer tensors to match exactly and ``num_objects``."""
    n_t = len(case["classes"])
    for i, s in enumerate(case["strides"]):
        for t in range(n_t):
            for k in ("classification_labels", "panoptics", "points_per_obj"):
                assert torch.equal(got[s][t][k].cpu(), ref[s][t][k]), (tag, s, t, k)
            r = got[s][t]["regression_targets"].cpu()
            # (1e-5 of the maximum, the bound of test_gpu_model.py: centre offsets of metres rotated with the device's sinf / cosf differ
            #  from the CPU's in the last fp32 bit, 5e-7 absolute)
            assert torch.isfinite(r).all() and rel_err(r, ref[s][t]["regression_targets"]) < 1e-5, (tag, s, t)
            assert int(nobj[i * n_t + t]) == ref[s][t]["num_objects"], (tag, s, t)


def _fixture_targets(g, case):
    ref = {}
    for s in case["strides"]:
        ref[s] = {}
        for t in range(len(case["classes"])):
            tg = {k: g[f"s{s}/t{t}/{k}"] for k in ("classification_labels", "panoptics", "regression_targets", "points_per_obj")}
            tg["num_objects"] = sum(int((x.unique() > 0).sum()) for x in tg["panoptics"])
            ref[s][t] = tg
    return ref


@pytest.mark.parametrize("name", list(CASES))
def test_targets_through_the_c_abi(golden, name):
    g0, g, case = golden("multilevel/common"), golden(f"multilevel/{name}"), CASES[name]
    got, nobj = _targets_through_the_c_abi(g0["cart"], g.np("annotations"), case)
    _assert_targets(got, nobj, _fixture_targets(g, case), case, name)


def test_targets_without_any_annotation():
    """m == 0: every output is background, no box buffer is touched."""
    import numpy as np

    case = CASES["D"]
    cart = torch.randn(2, 3, 8, 64)
    got, nobj = _targets_through_the_c_abi(cart, np.zeros((0, 13)), case)
    assert torch.equal(nobj, torch.zeros(4, dtype=torch.int32))
    for s in case["strides"]:
        for t, n in enumerate(case["classes"]):
            assert bool((got[s][t]["classification_labels"] == n).all()) and int(got[s][t]["panoptics"].abs().max()) == 0
            assert float(got[s][t]["regression_targets"].abs().max()) == 0.0 and int(got[s][t]["points_per_obj"].abs().max()) == 0


def _device_entries(entries):
    """Fixture entries -> device tensors; logits / regressands as leaves that want gradients; ``num_objects`` as the target kernel leaves it."""
    out = []
    for e in entries:
        tg = {k: v.to(DEV) for k, v in e["targets"].items()}
        tg["num_objects"] = torch.tensor([sum(int((x.unique() > 0).sum()) for x in e["targets"]["panoptics"])], dtype=torch.int32, device=DEV)
        out.append({"stride": e["stride"], "task": e["task"], "cart": e["cart"].to(DEV), "mask": e["mask"].to(DEV), "targets": tg,
                    "logits": e["logits"].to(DEV).requires_grad_(True), "regressands": e["regressands"].to(DEV).requires_grad_(True), "prefix": e["prefix"]})
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_loss_from_the_fixtures_logits(golden, name):
    """The two phases and the backward launch on the FIXTURE's fp32 logits / regressands (no tower rounding in the way): every key of the
    dict, soft targets, foreground, both gradients."""
    from range_view_3d_detection_amd.nn.heads.detection_head import DetectionHead

    g0, g, case = golden("multilevel/common"), golden(f"multilevel/{name}"), CASES[name]
    head = build_head(name)
    ents = _device_entries(case_entries(g0, g, name))
    outputs, data = {}, {}
    for e in ents:
        outputs.setdefault(e["stride"], {"cart": e["cart"], "mask": e["mask"]})[e["task"]] = {"logits": e["logits"], "regressands": e["regressands"]}
        data.setdefault(e["stride"], {})[e["task"]] = e["targets"]
    losses = DetectionHead.loss(head, outputs, data)
    ref = unpack(g, "loss")
    assert {k for k in losses if k != "aux"} == set(ref)
    for k, v in ref.items():
        assert abs(float(losses[k]) - float(v)) <= 1e-4 * max(abs(float(v)), 1e-3), (name, k, float(losses[k]), float(v))
    losses["loss"].backward()
    for e in ents:
        aux = losses["aux"][e["stride"]][e["task"]]
        assert torch.allclose(aux["targets"].cpu(), g[f"{e['prefix']}/soft"], atol=1e-5), (name, e["prefix"])
        assert aux["targets"] is data[e["stride"]][e["task"]]["targets"]
        assert torch.equal(aux["foreground"].cpu(), g[f"{e['prefix']}/foreground"]), (name, e["prefix"])
        for key, leaf in (("d_logits", e["logits"]), ("d_regressands", e["regressands"])):
            want = g[f"{e['prefix']}/{key}"]
            assert leaf.grad is not None and float((leaf.grad.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max()), (name, e["prefix"], key)


def test_one_entry_equals_the_one_level_entries_bit_for_bit(golden):
    """One level, one task through the new entry points against the existing ones on the same data: integer targets, soft targets,
    foreground and both gradients bit for bit, the normalisers and counts exactly; the atomically accumulated sums [0..11] and the scalars formed
    from them to 1e-12 (the order of the workgroups' additions is not fixed in either kernel)."""
    from range_view_3d_detection_amd.nn.heads import detection_head as dh

    g = golden("tiny_model")
    cart, ann = g["cart"].to(DEV), g.np("annotations")
    case = dict(strides=[1], classes=[5], method=None, partitions={1: [0.0, INF]})
    tasks = {0: [f"C{i}" for i in range(5)]}
    old = dh.compute_targets({"cart": cart, "annotations": ann}, tasks, [1], {"fpn_assignment_method": None})[1][0]
    new, nobj = _targets_through_the_c_abi(g["cart"], ann, case)
    for k in ("classification_labels", "panoptics", "points_per_obj"):
        assert torch.equal(old[k], new[1][0][k]), k
    # (the two target kernels are separate machine code: the compiler contracts the rotation's c * x + s * y into an fma on either
    #  product, so the encoded offsets agree to the last fp32 bit or the one before)
    assert rel_err(new[1][0]["regression_targets"], old["regression_targets"]) < 1e-6
    assert int(nobj[0]) == int(old["num_objects"])
    mask = g["mask"].to(DEV)
    res = {}
    for which in ("old", "new"):
        lg, rg = g["logits"].to(DEV).requires_grad_(True), g["regressands"].to(DEV).requires_grad_(True)
        flat = {k: old[k] for k in ("classification_labels", "panoptics", "regression_targets", "points_per_obj", "num_objects")}
        if which == "old":
            loss, sums, soft, fg = dh._DetectionLossFn.apply(lg, rg, cart, mask, flat, HP)
        else:
            ent = {"cart": cart, "mask": mask, "targets": flat}
            loss, sums = dh._MultiLevelLossFn.apply([ent], HP, lg, rg)
            soft, fg, sums = ent["soft"], ent["foreground"], sums[0]
        (3.0 * loss).backward()
        res[which] = (loss.detach(), sums.clone(), soft, fg, lg.grad, rg.grad)
    (l0, s0, soft0, fg0, dl0, dr0), (l1, s1, soft1, fg1, dl1, dr1) = res["old"], res["new"]
    assert torch.equal(soft0, soft1) and torch.equal(fg0, fg1) and torch.equal(dl0, dl1) and torch.equal(dr0, dr1)
    assert torch.equal(s0[[3, 12, 13]], s1[[3, 12, 13]])
    assert torch.allclose(s0[:12], s1[:12], rtol=1e-12, atol=0) and torch.allclose(s0[16:], s1[16:], rtol=1e-12, atol=0)
    assert torch.allclose(l0, l1, rtol=1e-12, atol=0)
    assert float(dl0.abs().max()) > 0 and float(dr0.abs().max()) > 0


def _load_twin(golden, name):
    from test_gpu_basic import build_basic

    g0, g = golden("multilevel/common"), golden(f"multilevel/{name}")
    backbone, _ = build_basic()
    head = build_head(name)
    backbone.load_state_dict({k[len("backbone."):]: v for k, v in unpack(g0, "sd").items()})
    head.load_state_dict({k[len("head."):]: v for k, v in unpack(g, "sd").items()})
    return g0, g, backbone.to(DEV), head.to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_twin_train_step(golden, name):
    """Backbone + multi-level head with the fixture's weights: masks and targets exact, tower outputs / loss within the bf16 bounds of
    tests/test_gpu_basic.py, parameter-gradient summaries of the towers against the reference's."""
    g0, g, backbone, head = _load_twin(golden, name)
    case = CASES[name]
    backbone.train(), head.train()
    data = {"features": g0["features"].to(DEV), "cart": g0["cart"].to(DEV), "mask": g0["mask"].to(DEV), "annotations": g.np("annotations")}
    outputs, losses = head(backbone(data), data, return_loss=True)
    for s in case["strides"]:
        assert torch.equal(outputs[s]["mask"].cpu(), g[f"s{s}/mask"]), (name, s)
        for t in range(len(case["classes"])):
            for k in ("classification_labels", "panoptics", "points_per_obj"):
                assert torch.equal(data[s][t][k].cpu(), g[f"s{s}/t{t}/{k}"]), (name, s, t, k)
            for k in ("logits", "regressands"):
                got, ref = outputs[s][t][k].float(), g[f"s{s}/t{t}/{k}"]
                assert got.shape == ref.shape and rel_err(got, ref) < 6e-2 and _cos(got, ref) > 0.985, (name, s, t, k, rel_err(got, ref))
    ref = unpack(g, "loss")
    assert rel_err(losses["loss"].reshape(()), ref["loss"].reshape(())) < 3e-2
    assert float(losses["total_objects"]) == float(ref["total_objects"])
    losses["loss"].backward()
    summ = unpack(g, "grad_summary")
    cosines, ratios = [], []
    for prefix, mod in (("backbone", backbone), ("head", head)):
        for k, p in mod.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (name, k)
            want = summ[f"{prefix}.{k}"].double()
            if float(want[0]) < 1e-9:
                continue
            got = grad_summary(f"{prefix}.{k}", p.grad.cpu())
            cosines.append(float((got[1:] @ want[1:]) / (got[1:].norm() * want[1:].norm() + 1e-30)))
            ratios.append(float(got[0] / want[0]))
    cosines.sort(), ratios.sort()
    n = len(cosines)
    print(f"    {name}: {n} parameters; projections' cosine median {cosines[n // 2]:.4f} q05 {cosines[n // 20]:.4f}; norm ratio median {ratios[n // 2]:.4f} "
          f"range {ratios[0]:.3f} .. {ratios[-1]:.3f}")
    # (norm + four random projections per parameter: they agree with the fp32 reference's as far as bf16 towers allow)
    assert cosines[n // 2] > 0.95 and cosines[n // 20] > 0.3, (name, cosines[n // 2], cosines[n // 20])
    assert 0.9 < ratios[n // 2] < 1.1 and ratios[n // 20] > 0.5 and ratios[n - 1 - n // 20] < 2.0, (name, ratios[n // 20], ratios[n // 2], ratios[n - 1 - n // 20])


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_twin_eval_and_decode(golden, name):
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

    g0, g, backbone, head = _load_twin(golden, name)
    case = CASES[name]
    backbone.eval(), head.eval()
    data = {"features": g0["features"].to(DEV), "cart": g0["cart"].to(DEV), "mask": g0["mask"].to(DEV)}
    tasks = {t: [f"T{t}C{i}" for i in range(n)] for t, n in enumerate(case["classes"])}
    with torch.no_grad():
        outputs, _ = head(backbone(data), data, return_loss=False)
    assert list(outputs.keys()) == case["strides"]
    dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    cfg = {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "WEIGHTED"}
    params, scores, cats, bidx = dec.decode(outputs, cfg, tasks, use_nms=False)
    ref_p, ref_s, ref_c, ref_b = g["eval/dec_params"], g["eval/dec_scores"], g["eval/dec_categories"], g["eval/dec_batch_index"]
    # every reference candidate whose score is clear of the threshold has a partner of the same sweep and category within half a metre
    # (bf16 towers against the fp32 reference; the fixture's tower outputs are rounded to 1/128, which is below that noise)
    clear = (ref_s - 0.1).abs() > 0.03
    d = torch.cdist(ref_p[clear][:, :3].double(), params.cpu()[:, :3].double())
    same = (ref_b[clear][:, None] == bidx.cpu()[None]) & (ref_c[clear][:, None] == cats.cpu()[None])
    found = ((d < 0.5) & same).any(dim=1)
    assert int(clear.sum()) > 10 and float(found.float().mean()) > 0.95, (name, int(found.sum()), int(clear.sum()))
    assert abs(scores.numel() - ref_s.numel()) <= 0.15 * ref_s.numel() + 2, (scores.numel(), ref_s.numel())
    if len(case["classes"]) > 1:  # category offsets of the second task
        n0 = case["classes"][0]
        assert int(ref_c.max()) >= n0 and int(cats.max()) == int(ref_c.max())
        assert abs(int((cats >= n0).sum()) - int((ref_c >= n0).sum())) <= 0.15 * int((ref_c >= n0).sum()) + 2
    # decode with NMS runs and keeps boxes of every level that had candidates
    p2, s2, c2, b2 = dec.decode(outputs, cfg, tasks, use_nms=True)
    assert p2.shape[1] == 10 and s2.numel() == c2.numel() == b2.numel() > 0 and int(c2.max()) < sum(case["classes"])
    per_level = []
    for s in case["strides"]:
        per_level.append(dec.decode({s: outputs[s]}, cfg, tasks, use_nms=False)[1].numel())
    print(f"    {name}: candidates per level {dict(zip(case['strides'], per_level))}, after NMS {s2.numel()}")
    assert sum(per_level) == scores.numel() and per_level[0] > 0, per_level


def test_no_host_synchronisation_in_head_loss_backward(golden):
    g0, g, backbone, head = _load_twin(golden, "D")
    backbone.train(), head.train()
    data = {"features": g0["features"].to(DEV), "cart": g0["cart"].to(DEV), "mask": g0["mask"].to(DEV), "annotations": g.np("annotations")}
    feats = backbone(data)
    outputs, losses = head(feats, dict(data), return_loss=True)  # warm-up: lazily built layers, library load
    losses["loss"].backward()
    torch.cuda.synchronize()
    feats = {k: v.detach().requires_grad_(True) for k, v in feats.items()}
    torch.cuda.set_sync_debug_mode("error")
    try:
        outputs, losses = head(feats, data, return_loss=True)
        losses["loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(feats[s].grad is not None for s in CASES["D"]["strides"]) and math.isfinite(float(losses["loss"]))


FULL = dict(strides=[1, 2, 4], classes=[3, 2], method="RANGE", partitions={1: [0.0, 15.0], 2: [15.0, 30.0], 4: [30.0, INF]})


def test_full_size_step():
    """rv-av2 widths, 4 x 64 x 2048, strides {1, 2, 4} RANGE x two tasks: targets equal the restatement exactly, the loss equals the
    restatement on the step's own logits, and one optimiser step through GradSync (one rank) moves every tower."""
    import test_multilevel_golden as host
    from bench import build_model, synthetic_batch
    from range_view_3d_detection_amd import engine as E

    batch = synthetic_batch(4, 64, 2048, seed=11, device="cpu", boxes_per_sweep=16, n_cls=2)
    ann = batch["annotations"].clone()
    ann[:, 10] = (torch.arange(ann.shape[0]) % 3 == 0).double()  # a third of the boxes to task 1; labels < 2 fit both tasks
    order = torch.argsort(ann[:, 12] * 2 + ann[:, 10], stable=True)  # rows sorted by (sweep, task)
    ann = ann[order]
    backbone, _ = build_model("rv-av2", 5)
    host.CASES["_full"] = FULL
    try:
        head = build_head("_full", tower_channels=512, fpn={1: 512, 2: 128, 4: 128})
    finally:
        del host.CASES["_full"]
    g = torch.Generator().manual_seed(5)
    for name, p in head.named_parameters():
        if name.endswith("0.weight"):
            p.data = 0.02 * torch.randn(p.shape, generator=g)
    backbone, head = backbone.to(DEV).train(), head.to(DEV).train()
    data = {k: (v.to(DEV) if k != "annotations" else ann) for k, v in batch.items()}
    params = [p for p in list(backbone.parameters()) + list(head.parameters()) if p.requires_grad]
    before = {k: p.detach().clone() for k, p in head.named_parameters()}
    opt = torch.optim.SGD(params, lr=1e-2)
    E.GRAD_SYNC = E.GradSync(params, 1)
    try:
        outputs, losses = head(backbone(data), data, return_loss=True)
        losses["loss"].backward()
        E.GRAD_SYNC.finish()
    finally:
        E.GRAD_SYNC = None
    opt.step()
    torch.cuda.synchronize()
    ref = restate_targets(batch["cart"], ann.numpy(), FULL["strides"], FULL["classes"], "RANGE", FULL["partitions"])
    entries = []
    for s in FULL["strides"]:
        dist = batch["cart"][:, :, :, ::s].norm(dim=1, keepdim=True)
        lower, upper = FULL["partitions"][s]
        mask_s = outputs[s]["mask"].cpu()  # (a norm within an ulp of a bound may fall on either side of it on the two machines)
        assert int((mask_s != (batch["mask"][:, :, :, ::s] & (dist > lower) & (dist <= upper))).sum()) <= 2, s
        for t, n_cls in enumerate(FULL["classes"]):
            for k in ("classification_labels", "panoptics", "points_per_obj"):
                assert torch.equal(data[s][t][k].cpu(), ref[s][t][k]), (s, t, k)
            assert rel_err(data[s][t]["regression_targets"], ref[s][t]["regression_targets"]) < 1e-5
            assert int(data[s][t]["num_objects"]) == ref[s][t]["num_objects"]
            entries.append({"n_cls": n_cls, "logits": outputs[s][t]["logits"].detach().float().cpu(), "regressands": outputs[s][t]["regressands"].detach().float().cpu(),
                            "cart": batch["cart"][:, :, :, ::s].contiguous(), "mask": mask_s, "targets": ref[s][t]})
    want, _ = restate_loss(entries, FULL["strides"])
    assert sum(ref[s][t]["num_objects"] for s in FULL["strides"] for t in range(2)) > 12
    for k, v in want.items():
        assert math.isfinite(float(losses[k])) and abs(float(losses[k]) - v) <= 1e-4 * max(abs(v), 1e-3), (k, float(losses[k]), v)
    moved = {k: not torch.equal(before[k], p.detach()) for k, p in head.named_parameters()}
    assert all(moved.values()), [k for k, m in moved.items() if not m]


# generation rv_tap_launch_info picks (256 compute units) per tower layer: [first layer from the level's channels, 3x3 at the head width,
# the 1x1 final with fp32 output] at 4 x 64 x (2048 / stride) -- DESIGN.md 5.2
CENSUS = {
    ("rv-av2", 1): (6, 6, 1), ("rv-av2", 2): (6, 6, 1), ("rv-av2", 4): (6, 6, 1), ("rv-av2", 16): (6, 6, 1),
    ("rv-waymo", 1): (6, 6, 1), ("rv-waymo", 2): (6, 6, 1), ("rv-waymo", 4): (6, 6, 1), ("rv-waymo", 16): (2, 2, 1),
}


@pytest.mark.parametrize("model,stride", list(CENSUS))
def test_tower_kernel_census(model, stride):
    from torch import nn

    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    level1, lower, width = {"rv-av2": (512, 128, 512), "rv-waymo": (256, 128, 256)}[model]
    w = 2048 // stride

    def generation(cin, cout, k, f32):
        layer = E.tap_layer(nn.Conv2d(cin, cout, k, padding=k // 2, bias=False))
        info = (ctypes.c_int32 * 4)()
        shape = L.TapShape(4, 64, w, w, cin, cout, L.OUT_F32 if f32 else 0)
        assert L.load().rv_tap_launch_info(ctypes.byref(layer.geom), ctypes.byref(shape), 0, info) == 0
        return info[0]

    got = (generation(level1 if stride == 1 else lower, width, 3, False), generation(width, width, 3, False), generation(width, 32, 1, True))
    assert got == CENSUS[(model, stride)], (model, stride, got)
