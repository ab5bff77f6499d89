"""The BASIC-stem models (base-av2 / base-waymo: the defaults of the reference's config tree) as composed models on the device.

* ``tests/golden/basic_model.npz`` (the reference's own RangeNet(stem_type="BASIC", layers [8, 8, 16, 16, 16]) + DetectionHead, BatchNorm
  gates open): state-dict keys, train forward / targets / loss / backward / running statistics, eval forward + decode with bf16 and
  fp16 operands, and the six-input-channel stem -- the twins of test_gpu_model.py's tiny-detector tests;
* base-av2 at full size (1 x 64 x 2048 and, as ``base-av2.yaml`` sets ``height: 32``, 1 x 32 x 2048), eval mode under fp16 autocast
  against the oracle, then decode + weighted NMS.
The real-width training steps are in test_gpu_realwidth.py / test_gpu_layerwise.py / test_gpu_fullsize_train.py, the kernels the
64-channel layers land on in test_gpu_tapconv2.py.
"""

from __future__ import annotations

import math

import pytest
import torch

from test_gpu_backward import _cos
from test_gpu_forward import DEV, rel_err
from test_oracle_golden import unpack  # (the fixture's state dicts are packed: tests/golden/make_golden.py ``pack``)

pytestmark = pytest.mark.gpu

NCLS = 5
WIDTHS = [8, 8, 16, 16, 16]


def build_basic(in_channels=5):
    from range_view_3d_detection_amd.nn.backbones.dla import RangeNet
    from range_view_3d_detection_amd.nn.heads.detection_head import DetectionHead

    c0 = WIDTHS[0]
    backbone = RangeNet(in_channels=in_channels, layers=list(WIDTHS), out_channels=c0, projection_kernel_size=1, dataset_name="av2",
                        num_neighbors=3, num_layers=2, stem_type="BASIC",
                        _net={"_target_": "torchbox3d.nn.backbones.dla.RangeBackbone", "in_channels": in_channels, "layers": list(WIDTHS), "out_channels": c0})
    tasks = {0: [f"C{i}" for i in range(NCLS)]}
    tcfg = {"dataset_name": "av2", "tasks": tasks, "enable_azimuth_invariant_targets": True, "range_partitions": {1: [0.0, math.inf]},
            "fpn_assignment_method": None, "k": math.inf, "affinity_fn": "GAUSSIAN", "normalize_affinities": False, "sigma": 0.75}
    head = DetectionHead(fpn={1: 2 * c0}, fpn_kernel_sizes={1: [3, 3]}, targets_config=tcfg, num_classification_blocks=4,
                         num_regression_blocks=4, final_kernel_size=1, tasks_cfg=tasks, task_in_channels=2 * c0, classification_weight=1.0,
                         regression_weight=1.0, coding_weights=[1.0] * 8, classification_head_channels=2 * c0,
                         regression_head_channels=2 * c0, classification_normalization_method="FOREGROUND",
                         _cls_loss={"_target_": "torchbox3d.nn.losses.classification.VarifocalLoss", "alpha": 0.75, "gamma": 2.0, "reduction": "none"},
                         _regression_loss={"_target_": "torch.nn.L1Loss", "reduction": "none"})
    return backbone, head


def load_basic(g):
    backbone, head = build_basic()
    sd = unpack(g, "sd")
    backbone.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")})
    head.load_state_dict({k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")})
    return backbone.to(DEV), head.to(DEV)


def test_state_dict_keys_match_reference_and_the_stem_is_a_basic_block(golden):
    from range_view_3d_detection_amd.nn.blocks import BasicBlock

    g = golden("basic_model")
    backbone, head = build_basic()
    ours = {f"backbone.{k}" for k in backbone.state_dict()} | {f"head.{k}" for k in head.state_dict()}
    ref = unpack(g, "sd")
    assert ours == set(ref)
    assert isinstance(backbone.stem, BasicBlock) and backbone.stem.projection_block is not None
    assert {k: tuple(v.shape) for k, v in backbone.state_dict().items()} == {k[len("backbone."):]: tuple(v.shape) for k, v in ref.items() if k.startswith("backbone.")}


def test_basic_detector_forward_backward(golden):
    """Train forward, targets, loss, backward and running statistics against the reference's arrays, with the CPU bf16 emulation's own
    distance from them as the yardstick (as test_gpu_model.py::test_tiny_detector_forward_backward).  The fixture's ReLU gates are open,
    so -- unlike the tiny model's -- its parameter gradients are comparable across precisions: per-parameter cosine against the fp32
    oracle's gradients (pinned to the reference by tests/test_oracle_golden.py; the fixture stores summaries of them) no worse than
    the emulation's (median - 0.02, 5 % quantile - 0.05)."""
    import numpy as np

    from oracle import model as om
    from oracle import targets as otgt

    g = golden("basic_model")
    backbone, head = load_basic(g)
    backbone.train(), head.train()
    data = {"features": g["features"].to(DEV), "cart": g["cart"].to(DEV), "mask": g["mask"].to(DEV), "annotations": g["annotations"]}
    sd = unpack(g, "sd")
    tg = otgt.compute_targets(g["cart"], g["annotations"], NCLS)

    def oracle_run(nm):
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
        f, lg, rg = om.detector_forward(g["features"], g["cart"], {**sd, **p}, stem_type="BASIC", nm=nm)
        otgt.detection_loss(lg, rg, g["cart"], g["mask"], tg, NCLS)["loss"].backward()
        return f, lg, rg, p

    feats_o, logits_o, reg_o, params = oracle_run(om.Numerics.bf16(train=True))
    *_, params32 = oracle_run(om.Numerics(train=True))
    feats = backbone(data)
    outputs, losses = head(feats, data, return_loss=True)
    pairs = [(f"feat/{s}", feats[s].float(), feats_o[s].detach(), g[f"feat/{s}"]) for s in (1, 2, 4, 16)]
    pairs += [("logits", outputs[1][0]["logits"], logits_o.detach(), g["logits"]), ("regressands", outputs[1][0]["regressands"], reg_o.detach(), g["regressands"])]
    for name, got, orc, ref in pairs:
        assert got.shape == ref.shape, name
        emu = rel_err(orc, ref)
        e_ref, e_orc = rel_err(got, ref), rel_err(got, orc)
        print(f"basic detector {name}: emulation {emu:.3e}, HIP vs fp32 {e_ref:.3e}, HIP vs emulation {e_orc:.3e}")
        assert e_orc < max(3e-2, 2.0 * emu + 1e-2) and _cos(got, orc) > 0.99, (name, e_orc, emu)
        assert e_ref < max(3e-2, 1.5 * emu + 1e-2) and _cos(got, ref) > 0.985, (name, e_ref, emu)
    for k in ("classification_labels", "panoptics", "points_per_obj"):
        assert torch.equal(data[1][0][k].cpu(), g[f"targets/{k}"])
    assert rel_err(losses["loss"].reshape(()), unpack(g, "loss")["loss"].reshape(())) < 3e-2
    losses["loss"].backward()
    cos_hip, cos_emu = [], []
    for prefix, mod in (("backbone", backbone), ("head", head)):
        for k, p in mod.named_parameters():
            ref = params32[f"{prefix}.{k}"].grad
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
            if float(ref.norm()) < 1e-9:
                continue
            cos_hip.append(_cos(p.grad.cpu(), ref))
            cos_emu.append(_cos(params[f"{prefix}.{k}"].grad, ref))
    med, q, med_e, q_e = np.median(cos_hip), np.quantile(cos_hip, 0.05), np.median(cos_emu), np.quantile(cos_emu, 0.05)
    print(f"    {len(cos_hip)} parameters; gradient cosine vs the fp32 oracle: HIP median {med:.4f} q05 {q:.4f}; CPU bf16 emulation {med_e:.4f} / {q_e:.4f}")
    assert med > med_e - 0.02 and q > q_e - 0.05, (med, med_e, q, q_e)
    sd_after = {**{f"backbone.{k}": v for k, v in backbone.state_dict().items()}, **{f"head.{k}": v for k, v in head.state_dict().items()}}
    worst = max(rel_err(sd_after[k], v) for k, v in unpack(g, "sd_after").items())
    assert worst < 5e-2, worst


@pytest.mark.parametrize("operand", ["bf16", "f16"])
def test_basic_detector_eval_and_decode(golden, operand):
    import contextlib

    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

    g = golden("basic_model")
    backbone, head = load_basic(g)
    backbone.eval(), head.eval()
    data = {"features": g["features"].to(DEV), "cart": g["cart"].to(DEV), "mask": g["mask"].to(DEV)}
    with torch.no_grad(), (torch.autocast("cuda", dtype=torch.float16) if operand == "f16" else contextlib.nullcontext()):
        feats = backbone(data)
        outputs, _ = head(feats, data, return_loss=False)
    assert feats[1].dtype == (torch.float16 if operand == "f16" else torch.bfloat16)
    bound = 1e-2 if operand == "f16" else 6e-2  # (bf16: the tiny detector's bound; fp16 has three more mantissa bits)
    assert rel_err(outputs[1][0]["logits"], g["eval/logits"]) < bound
    assert rel_err(outputs[1][0]["regressands"], g["eval/regressands"]) < bound
    dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    post = {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "WEIGHTED"}
    mo = {1: {"cart": data["cart"], "mask": data["mask"], 0: {"logits": g["eval/logits"].to(DEV), "regressands": g["eval/regressands"].to(DEV)}}}
    p, s, c, b = dec.decode(mo, post, {0: ["c"] * NCLS}, use_nms=False)
    assert torch.equal(c.cpu(), g["eval/dec_categories"]) and torch.equal(b.cpu(), g["eval/dec_batch_index"])
    assert rel_err(p, g["eval/dec_params"]) < 1e-5 and rel_err(s, g["eval/dec_scores"]) < 1e-6
    p, s, c, b = dec.decode(outputs, post, {0: ["c"] * NCLS}, use_nms=True)
    assert p.shape[1] == 10 and p.shape[0] == s.shape[0] == c.shape[0] == b.shape[0] and p.shape[0] > 0
    assert torch.isfinite(p).all() and (s >= 0).all()


def test_range_net_dispatches_to_the_basic_stem_with_six_input_channels(golden):
    """RangeNet(stem_type="BASIC", in_channels=6) (nn/backbones/dla.py: the BASIC arm of the stem dispatch) in eval and in train mode
    against the reference: the stem's eval output, and the train-mode feature maps at all four strides."""
    g = golden("basic_model")
    net, _ = build_basic(in_channels=6)
    sd = {k[len("backbone."):]: v for k, v in unpack(g, "sd").items() if k.startswith("backbone.net.")}
    sd.update(unpack(g, "c6/sd"))
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    data = {"features": g["c6/features"].to(DEV), "cart": g["c6/cart"].to(DEV), "mask": g["c6/mask"].to(DEV)}
    with torch.no_grad():
        out = net(data)
    assert rel_err(out[1][:, :8].float(), g["c6/eval_stem"]) < 5e-2  # (level 1 = [stem, agg3]: its first half is the stem's output)
    out = net.train()(data)
    for s_, ref in g.sub("c6/feat").items():
        assert rel_err(out[int(s_)].float(), ref) < 5e-2 and _cos(out[int(s_)].float(), ref) > 0.999, (s_, rel_err(out[int(s_)].float(), ref))


@pytest.mark.parametrize("H", [64, 32])
def test_base_av2_full_size_eval_forward_fp16_vs_oracle_and_decode(H):
    """base-av2 at 1 x H x 2048 in eval mode under fp16 autocast (what the reference's validation step runs), library's own kernel
    selection: logits / regressands against the fp32 oracle and its fp16 emulation (bound of the rv-av2 test: 4e-3 of the maximum), the
    decoded candidates against the oracle decoder on the same logits, and decode + weighted NMS against the oracle NMS on the device's
    candidates.  H = 32 is the height ``conf/experiment/base-av2.yaml`` sets: every count of tile rows changes."""
    from oracle import decode as odec
    from oracle import model as om
    from oracle import nms as onms
    from range_view_3d_detection_amd import engine as E
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder, decode_candidates
    from test_gpu_nms_wrapper import _canonical
    from test_gpu_realwidth import _prepare

    backbone, head, sd, batch = _prepare("base-av2", 5, 26, 2048, 0.5, H=H)
    head.classification_head["1"]["0"].blocks[-1][0].bias.data.fill_(-1.5)  # some scores above min_confidence
    sd["head.classification_head.1.0.blocks.4.0.bias"] = head.classification_head["1"]["0"].blocks[-1][0].bias.data.clone()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        _, lg32, rg32 = om.detector_forward(batch["features"], batch["cart"], sd, stem_type="BASIC", nm=om.Numerics(train=False))
        _, lg16, rg16 = om.detector_forward(batch["features"], batch["cart"], sd, stem_type="BASIC", nm=om.Numerics.fp16(train=False))
    backbone, head = backbone.to(DEV).eval(), head.to(DEV).eval()
    data = {k: (v.to(DEV) if k != "annotations" else v) for k, v in batch.items()}
    E.PROFILE = E.KernelProfile()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            feats = backbone(data)
            outputs, _ = head(feats, data, return_loss=False)
        torch.cuda.synchronize()
        ran = set(name for name, *_ in E.PROFILE.records)
    finally:
        E.PROFILE = None
    assert feats[1].dtype == torch.float16
    assert "tapconv2_kernel<2>" in ran and any(n.startswith(("tapconv5_kernel<", "tapconv6_kernel<")) for n in ran), sorted(ran)
    logits, reg = outputs[1][0]["logits"].float().cpu(), outputs[1][0]["regressands"].float().cpu()
    m = {"logits~fp16": rel_err(logits, lg16), "logits~fp32": rel_err(logits, lg32), "emu~fp32": rel_err(lg16, lg32),
         "reg~fp16": rel_err(reg, rg16), "reg~fp32": rel_err(reg, rg32), "reg emu~fp32": rel_err(rg16, rg32)}
    print(f"[base-av2 eval 1x{H}x2048, fp16 operands] " + "  ".join(f"{k} {v:.3e}" for k, v in m.items()) + f"  kernels {sorted(ran)}")
    for k in ("logits~fp16", "logits~fp32", "reg~fp16", "reg~fp32"):
        assert m[k] < 4e-3, m
    dec = RangeDecoder(True, True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    post = {"num_pre_nms": 50000, "num_post_nms": 1000, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "WEIGHTED"}
    o = outputs[1][0]
    sc, ct, bx = decode_candidates(o["logits"], o["regressands"], data["cart"], data["mask"], True, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    sco, cto, bxo = odec.dense_candidates(logits, reg, batch["cart"], batch["mask"])
    assert rel_err(sc, sco) < 1e-6 and rel_err(bx, bxo) < 1e-5
    assert float((ct.cpu() != cto).float().mean()) < 1e-4
    p, s, c, b = dec.decode(outputs, post, {0: [f"C{i}" for i in range(26)]}, use_nms=True)
    bo_, so, co, io = onms.batched_multiclass_nms(bx.cpu(), sc.cpu(), ct.cpu(), 50000, 1000, 0.3, 0.1)
    po = torch.cat([bo_[:, :-1], odec.yaw_to_quat(bo_[:, -1:])], dim=-1)
    assert p.shape[0] > 20 and p.shape == po.shape, (p.shape, po.shape)
    p, s, c, b = _canonical(p, s, c, b)
    po, so, co, io = _canonical(po, so, co, io)
    assert torch.equal(c, co) and torch.equal(b, io)
    assert rel_err(p, po) < 1e-5 and rel_err(s, so) < 1e-6, (rel_err(p, po), rel_err(s, so))
