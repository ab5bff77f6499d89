"""Life cycle of the cached device images: one model run in one mode, changed, and run again.

``engine.TapLayer`` keeps every image made from parameters in one cache, ``layer.images`` (``images.ImageCache``): packed weight images of
both operand types, the persistent buffers the batched re-pack writes, the folded stride-1 images, the eval-mode BatchNorm folds (weight
image + padded bias per (form, operand)) and the padded bias; ``program.py`` keeps host copies of the ``RangePartition`` bounds.  All of them
are kept valid by one rule, ``images.source_key``: the version counter and the pointer of every tensor the image was made from.  A wrong image
makes no kernel test fail; it shows as validation outputs that are silently wrong.  Two checking layers, used by every scenario:

* ``audit(model)``: every entry of ``layer.images.entries()`` that the layer would SERVE now is re-made from the entry's recorded source
  tensors through a fresh ``TapLayer`` with an empty cache and must be equal bit for bit (the pack kernels are tested against torch
  elsewhere: here the fresh pack is the reference for staleness only).  A weight image whose key no longer matches the parameter (all of them right after an optimiser step)
  is not served -- it is re-packed at its next use -- and is counted under ``stale_skipped``.  The audit never re-packs the weight images or
  the folded images itself, so it can run between training steps without taking work away from ``prepack_stale``.
* ``cold(model)``: a new model that has never run, loaded with a deep copy of the warm model's state dict.  The warm model's eval outputs
  must EQUAL the cold model's (``torch.equal``); two cold rebuilds are shown to be bit-equal first, so a mismatch means staleness.
* the state dict read back from the device goes through the CPU oracle in eval mode (fp32): ``rel_err(warm, oracle)`` within
  ``1.5 x yardstick + 1e-2`` (the convention of tests/test_gpu_realwidth.py; yardstick = fp32 oracle against the bf16- / fp16-emulating oracle on
  the same state dict, measured here), and -- the teeth -- the oracle's output on the state before the event differs from the one after it by more
  than three times that bound: a stale image could not hide inside the tolerance.
"""

from __future__ import annotations

import contextlib
import copy
import gc
import types

import pytest
import torch

from test_gpu_forward import DEV, rel_err

pytestmark = pytest.mark.gpu

N_CLS = 3
KINDS = ("packed", "packed_f16", "fold", "fold_f16", "eval_fold", "eval_fold_folded", "bias_pad")  # (eval_fold_folded: those of eval_fold in the folded strided form)


# ---------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------
def _randomise(model, seed):
    """BatchNorm tensors as tests/test_gpu_realwidth.py::_prepare draws them (ReLU gates firmly open: bias around 3); the towers' conv weights
    as ``smoke()`` draws them (std 0.08: with the initialisation's near-zero final convs both outputs are their biases, whatever comes before)."""
    gen = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        if "_head." in name and name.endswith("0.weight"):
            p.data = 0.08 * torch.randn(p.shape, generator=gen)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=gen)
            m.bias.data = 0.2 * torch.randn(m.bias.shape, generator=gen) + 3.0
            m.running_mean.data = 0.1 * torch.randn(m.running_mean.shape, generator=gen)
            m.running_var.data = 0.5 + torch.rand(m.running_var.shape, generator=gen)
    return model


def build(widths, seed=0):
    from bench import Detector, build_model

    torch.manual_seed(seed)
    backbone, head = build_model(widths, N_CLS)
    return _randomise(Detector(backbone, head), seed + 1).to(DEV)


def batch_of(B, H, W, seed):
    from bench import synthetic_batch

    return synthetic_batch(B, H, W, seed=seed, device=DEV, boxes_per_sweep=4, n_cls=N_CLS)


def state_of(model):
    """The model's state dict read back from the device (cloned, CPU)."""
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def cold(model, widths):
    """A model that has never run, carrying a deep copy of ``model``'s current state."""
    from bench import Detector, build_model

    backbone, head = build_model(widths, N_CLS)
    fresh = Detector(backbone, head)
    fresh.load_state_dict(copy.deepcopy(state_of(model)))
    return fresh.to(DEV)


def _grids(small):
    from range_view_3d_detection_amd import _lib as L

    return L.select(L.SEL_SMALL_GRIDS) if small else contextlib.nullcontext()


def evaluate(model, batch, tag="bf16", small=False):
    """Eval-mode forward: (logits, regressands) as fp32 CPU tensors.  ``tag`` "f16": under ``torch.autocast("cuda", dtype=torch.float16)``."""
    model.eval()
    data = dict(batch)
    cast = torch.autocast("cuda", dtype=torch.float16) if tag == "f16" else contextlib.nullcontext()
    with torch.no_grad(), cast, _grids(small):
        out, _ = model.head(model.backbone(data), data, return_loss=False)
    lg, rg = out[1][0]["logits"].float().cpu(), out[1][0]["regressands"].float().cpu()
    assert torch.isfinite(lg).all() and torch.isfinite(rg).all()
    return lg, rg


def optimiser(model, lr=2e-3):
    """The recipe's fused AdamW over the parameters that take gradients (no scheduler: a first step moves every weight by about ``lr`` --
    2 to 5 % of a typical weight of these models, a bf16 ulp being 0.4 % -- so a stale image cannot equal a fresh one by rounding)."""
    from range_view_3d_detection_amd.nn.meta.arch import configure_optimizers

    params = [p for p in model.parameters() if p.requires_grad]
    return configure_optimizers(params, num_devices=1, batch_size=2, total_steps=100, lr=lr, debug=True, fused=True, max_grad_norm=35.0)[0]


def train(model, opt, batches, small=False, between=None):
    """Full training steps.  ``between``: called after backward and before the optimiser writes the parameters -- the moment at which the
    images the step ran on (those of ``prepack_stale`` among them) are current."""
    model.train()
    with _grids(small):
        for b in batches:
            opt.zero_grad(set_to_none=True)
            loss = model(b)
            loss.backward()
            if between is not None:
                between()
            opt.step()
    assert torch.isfinite(loss.detach())


# ---------------------------------------------------------------------------------------------
# layer 1: cache audit
# ---------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))


def layers_of(model):
    """(module name, TapLayer) of every conv of ``model`` that has run."""
    return [(name, m.__dict__["_rv_layer"]) for name, m in model.named_modules() if "_rv_layer" in m.__dict__]


def audit(model):
    """Every cached image the conv layers of ``model`` would serve now against a fresh pack of the current parameters; returns the number
    of images compared per kind (and ``stale_skipped``: weight images whose key says "re-pack at next use")."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    n = dict.fromkeys(KINDS + ("stale_skipped",), 0)
    f16 = {"bf16": "", "f16": "_f16"}
    modules = dict(model.named_modules())
    with torch.no_grad():
        for name, l in layers_of(model):
            assert l.weight is modules[name].weight, name
            g = l.geom
            for e in l.images.entries():
                kind, form, tag = e.slot
                what = (name, e.slot)
                # the fresh layer is built from the tensors the entry says it was made from: they must be the layer's own
                assert e.sources[0] is (l.bias if kind == "bias" else l.weight), what
                fresh = E.TapLayer(l.weight if kind == "bias" else e.sources[0], g.stride_w, (g.pad_h, g.pad_w), l.transposed,
                                   bias=e.sources[0] if kind == "bias" else l.bias, in_perm=l.in_perm)
                if kind in ("weight", "folded"):
                    if not e.current:
                        n["stale_skipped"] += 1
                        continue
                    with L.operand(tag):
                        assert _same_bits(e.data, fresh.packed(form)), what
                    n[("packed" if kind == "weight" else "fold") + f16[tag]] += 1
                elif kind == "eval_fold":
                    assert len(e.sources) == 5 and len(e.extra) == 1, what
                    bn = types.SimpleNamespace(**dict(zip(("weight", "bias", "running_mean", "running_var"), e.sources[1:])), eps=e.extra[0])
                    with L.operand(tag):
                        img, bias = l.packed_eval(form, bn)  # what the layer serves for the current state of conv and BatchNorm
                        ref_img, ref_bias = fresh.packed_eval(form, bn)
                    assert _same_bits(img, ref_img), what + ("image",)
                    assert bias.dtype == torch.float32 and torch.equal(bias, ref_bias), what + ("bias",)
                    n["eval_fold"] += 1
                    n["eval_fold_folded"] += int(form == "folded")
                else:
                    assert kind == "bias" and torch.equal(l.padded_bias(), fresh.padded_bias()), what
                    n["bias_pad"] += 1
    return n


def expect(counts, *kinds):
    for k in kinds:
        assert counts[k] > 0, (k, counts)


# ---------------------------------------------------------------------------------------------
# layer 2: warm model against a cold rebuild and the oracle
# ---------------------------------------------------------------------------------------------
def oracle_eval(sd, batch, numerics=None):
    from oracle import model as om

    with torch.no_grad():
        _, lg, rg = om.detector_forward(batch["features"].cpu(), batch["cart"].cpu(), sd, nm=numerics or om.Numerics(train=False))
    return lg, rg


def check_cold_rebuilds_agree(model, widths, batch, tags=("bf16",), small=False):
    """Precondition: two cold rebuilds of one state dict give bit-equal eval outputs -- a later mismatch is staleness, not noise."""
    for tag in tags:
        a, b = evaluate(cold(model, widths), batch, tag, small), evaluate(cold(model, widths), batch, tag, small)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tag


def check_warm(model, widths, batch, tag="bf16", small=False, before=None, label=""):
    """Warm model == cold rebuild bit for bit; warm model within the project's bound of the fp32 oracle on its own state dict; and, with
    ``before`` (the oracle's fp32 outputs on the state before the event), the event moved the outputs by more than 3 x that bound.
    Returns (warm outputs, the oracle's fp32 outputs on the current state)."""
    from oracle import model as om

    warm = evaluate(model, batch, tag, small)
    ref = evaluate(cold(model, widths), batch, tag, small)
    for w, c, what in zip(warm, ref, ("logits", "regressands")):
        assert torch.equal(w, c), (label, tag, what, "warm model differs from its cold rebuild", rel_err(w, c))
    sd = state_of(model)
    o32 = oracle_eval(sd, batch)
    o16 = oracle_eval(sd, batch, om.Numerics.fp16(train=False) if tag == "f16" else om.Numerics.bf16(train=False))
    for i, what in enumerate(("logits", "regressands")):
        bound = 1.5 * rel_err(o16[i], o32[i]) + 1e-2
        err = rel_err(warm[i], o32[i])
        moved = rel_err(before[i], o32[i]) if before is not None else float("nan")
        print(f"[{label} {tag}] {what}: warm~fp32 {err:.3e}  bound {bound:.3e}  event moved the oracle by {moved:.3e}")
        assert err < bound, (label, tag, what, err, bound)
        if before is not None:
            assert moved > 3.0 * bound, (label, tag, what, "the event is inside the tolerance: it proves nothing", moved, bound)
    return warm, o32


# ---------------------------------------------------------------------------------------------
# running statistics at model level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", ["c32", "c24"])
def test_running_statistics_after_three_training_forwards_vs_oracle(widths):
    """Three train-mode forwards of the whole detector on three seeded batches: every ``running_mean`` / ``running_var`` against the oracle
    stepping the same batches (``Numerics(train=True)``, ``nm.running`` fed forward), ``num_batches_tracked == 3`` everywhere.  c32: the
    kernels update the module's tensors in place; c24: padded copies written back with ``copy_``.  Bound per tensor: 1.5 x |fp32 oracle -
    bf16-emulating oracle| (max over the tensor) + 1e-3 of the tensor's maximum.
    Largest measured ratio error / bound on MI355X: c32 0.705, c24 0.592."""
    from oracle import model as om

    model = build(widths)
    sd0 = state_of(model)
    batches = [batch_of(2, 16, 64, seed) for seed in (11, 12, 13)]
    model.train()
    with torch.no_grad():
        for b in batches:
            model(b)
    got = state_of(model)

    def stepped(make):
        sd = dict(sd0)
        with torch.no_grad():
            for b in batches:
                nm = make()
                om.detector_forward(b["features"].cpu(), b["cart"].cpu(), sd, nm=nm)
                assert nm.running
                sd.update(nm.running)
        return sd

    o32 = stepped(lambda: om.Numerics(train=True, running={}))
    o16 = stepped(lambda: om.Numerics.bf16(train=True))
    worst, n = (0.0, ""), 0
    for k, v in got.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3, k
        if "running_" not in k:
            continue
        assert not torch.equal(v, sd0[k]), k
        err = float((v.double() - o32[k].double()).abs().max())
        bound = 1.5 * float((o16[k].double() - o32[k].double()).abs().max()) + 1e-3 * float(o32[k].abs().max())
        worst = max(worst, (err / bound, k))
        n += 1
        assert err <= bound, (k, err, bound)
    assert n == 2 * sum(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules()) and n > 100
    print(f"[{widths}] {n} running statistics; largest error / bound {worst[0]:.3f} ({worst[1]})")


# ---------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------
CASES = [("c32", 64, False), ("c128", 128, True)]


def test_eval_reestimate_eval():
    """1. eval -> three train-mode forwards under ``torch.no_grad()`` with no optimiser (BatchNorm re-estimation: SWA's ``update_bn``) -> eval.
    No parameter changes; only the running statistics do, written by the kernels through raw pointers."""
    model = build("c32")
    batch = batch_of(2, 16, 64, 3)
    check_cold_rebuilds_agree(model, "c32", batch)
    _, o_before = check_warm(model, "c32", batch, label="1 first eval")
    expect(audit(model), "packed", "eval_fold", "bias_pad")
    model.train()
    with torch.no_grad():
        for seed in (21, 22, 23):
            model(batch_of(2, 16, 64, seed))
    check_warm(model, "c32", batch, before=o_before, label="1 after re-estimation")
    expect(audit(model), "packed", "eval_fold", "bias_pad")


@pytest.mark.parametrize("widths,W,small,whole", [(*c, False) for c in CASES] + [("c32", 64, False, True)])
def test_frozen_backbone_convs(widths, W, small, whole):
    """2. Every conv of the backbone frozen (``requires_grad_(False)``), BatchNorm in train mode, the optimiser holds the rest: two full
    steps -> eval.  The frozen convs' weights never change; the BatchNorms behind them do.  ``whole``: the BatchNorms' weights and biases
    are frozen as well (a frozen feature extractor whose statistics still adapt): then NO tensor torch sees changing feeds the backbone's
    folds -- only the running statistics the kernels write do."""
    model = build(widths)
    batch = batch_of(2, 16, W, 3)
    check_cold_rebuilds_agree(model, widths, batch, small=small)
    _, o_before = check_warm(model, widths, batch, small=small, label="2 first eval")
    for m in model.backbone.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            m.requires_grad_(False)
    if whole:
        model.backbone.requires_grad_(False)
    frozen = {k: v.clone() for k, v in model.backbone.state_dict().items() if k.endswith("conv.weight")}
    train(model, optimiser(model), [batch_of(2, 16, W, 31), batch_of(2, 16, W, 32)], small,
          between=lambda: expect(audit(model), "packed", "bias_pad", *(("fold",) if small else ())))
    assert all(torch.equal(v, model.backbone.state_dict()[k]) for k, v in frozen.items())
    check_warm(model, widths, batch, small=small, before=o_before, label="2 after two steps")
    expect(audit(model), "packed", "eval_fold", "bias_pad", *(("eval_fold_folded",) if small else ()))


@pytest.mark.parametrize("widths,W,small", CASES)
def test_ordinary_loop_alternating_operand_types(widths, W, small):
    """3. eval (bf16) -> two optimiser steps -> eval (f16 autocast) -> two steps -> eval (bf16) -> eval (f16): the fp16 weight images
    and the fp16 folds neither survive a re-pack nor are lost to ``prepack_stale``; inside every training step (after backward) the images the
    step ran on -- the folded images of the strided layers among them at c128 -- are audited while they are current."""
    model = build(widths)
    batch = batch_of(2, 16, W, 3)
    check_cold_rebuilds_agree(model, widths, batch, ("bf16", "f16"), small)
    opt = optimiser(model)
    folded = ("eval_fold_folded",) if small else ()  # (c128 under SEL_SMALL_GRIDS: the strided layers run in their folded stride-1 form)
    in_step = lambda: expect(audit(model), "packed", "bias_pad", *(("fold",) if small else ()))
    _, o = check_warm(model, widths, batch, "bf16", small, label="3 first eval")
    expect(audit(model), "packed", "eval_fold", "bias_pad", *folded)
    train(model, opt, [batch_of(2, 16, W, 41), batch_of(2, 16, W, 42)], small, between=in_step)
    _, o = check_warm(model, widths, batch, "f16", small, before=o, label="3 after steps 1-2")
    expect(audit(model), "packed_f16", "eval_fold", "bias_pad", *folded)
    train(model, opt, [batch_of(2, 16, W, 43), batch_of(2, 16, W, 44)], small, between=in_step)
    _, o = check_warm(model, widths, batch, "bf16", small, before=o, label="3 after steps 3-4")
    expect(audit(model), "packed", "eval_fold", "bias_pad", *folded)
    check_warm(model, widths, batch, "f16", small, label="3 last eval")
    expect(audit(model), "packed", "packed_f16", "eval_fold", "bias_pad", *folded)
    # both operand types' folds are held at once
    tags = {e.slot[2] for _, l in layers_of(model) for e in l.images.entries() if e.slot[0] == "eval_fold" and e.current}
    assert tags == {"bf16", "f16"}, tags


def test_checkpoint_into_a_warm_model():
    """4. Train two steps, eval, ``load_state_dict`` of a differently seeded checkpoint: eval equals that checkpoint's cold model; the first
    checkpoint loaded again gives the first eval bit for bit."""
    model = build("c32")
    batch = batch_of(2, 16, 64, 3)
    check_cold_rebuilds_agree(model, "c32", batch)
    train(model, optimiser(model), [batch_of(2, 16, 64, 51), batch_of(2, 16, 64, 52)])
    first, o_first = check_warm(model, "c32", batch, label="4 trained")
    ckpt_a = copy.deepcopy(state_of(model))
    ckpt_b = state_of(build("c32", seed=7))
    model.load_state_dict(ckpt_b)
    _, o_b = check_warm(model, "c32", batch, before=o_first, label="4 other checkpoint")
    expect(audit(model), "packed", "eval_fold", "bias_pad")
    model.load_state_dict(ckpt_a)
    again, _ = check_warm(model, "c32", batch, before=o_b, label="4 first checkpoint again")
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    expect(audit(model), "packed", "eval_fold", "bias_pad")


def _edit_targets(model):
    """A conv and a BatchNorm of the backbone; the biased final conv and the first BatchNorm of the classification tower."""
    blk = model.head.classification_head["1"]["0"].blocks
    res = model.backbone.net.res2
    conv = next(m for m in res.modules() if isinstance(m, torch.nn.Conv2d))
    bn = next(m for m in res.modules() if isinstance(m, torch.nn.BatchNorm2d))
    return conv, bn, blk[-1][0], blk[0][1]


def test_in_place_edits_torch_can_see():
    """5. ``mul_(1.01)`` and ``copy_`` on a conv weight, a conv bias and a BatchNorm weight, ``fill_`` on ``running_var``: each is picked up by
    the next forward.  (1.01 is more than a bf16 ulp, but far less than the oracle comparison resolves: every single edit is held to
    "outputs changed" + audit + bit equality with the cold rebuild; the oracle comparison with its 3 x bound teeth spans the whole sequence.)"""
    model = build("c32")
    batch = batch_of(2, 16, 64, 3)
    check_cold_rebuilds_agree(model, "c32", batch)
    last, o_before = check_warm(model, "c32", batch, label="5 first eval")
    conv, bn, final, tower_bn = _edit_targets(model)
    reg = model.head.regression_head["1"]["0"].blocks
    gen = torch.Generator().manual_seed(5)
    edits = []
    for what, p in (("conv weight", conv.weight), ("conv bias", final.bias), ("BatchNorm weight", bn.weight), ("tower BatchNorm weight", tower_bn.weight),
                    ("regression conv bias", reg[-1][0].bias), ("regression tower BatchNorm weight", reg[0][1].weight)):
        # (copy_ first: the regression tower's final bias is initialised to zero, and 1.01 x 0 is no edit)
        edits.append((what + " copy_", lambda p=p: p.copy_((0.5 * max(float(p.abs().mean()), 0.1) * (1.0 + torch.rand(p.shape, generator=gen))).to(DEV))))
        edits.append((what + " mul_", lambda p=p: p.mul_(1.01)))
    edits.append(("running_var fill_", lambda: bn.running_var.fill_(4.0)))
    edits.append(("tower running_var fill_", lambda: tower_bn.running_var.fill_(4.0)))
    edits.append(("regression tower running_var fill_", lambda: reg[0][1].running_var.fill_(4.0)))
    for what, edit in edits:
        with torch.no_grad():
            edit()
        warm = evaluate(model, batch)
        assert not (torch.equal(warm[0], last[0]) and torch.equal(warm[1], last[1])), (what, "the edit did not reach the outputs")
        ref = evaluate(cold(model, "c32"), batch)
        assert torch.equal(warm[0], ref[0]) and torch.equal(warm[1], ref[1]), (what, rel_err(warm[0], ref[0]), rel_err(warm[1], ref[1]))
        expect(audit(model), "packed", "eval_fold", "bias_pad")
        last = warm
    check_warm(model, "c32", batch, before=o_before, label="5 after all edits")


def test_edits_torch_cannot_see_then_invalidate():
    """6. ``p.data.add_(...)`` on conv weights, a conv bias, BatchNorm weights and running statistics, then
    ``engine.invalidate_packed_weights(model)``: after the call the audit and the cold equality hold, under both operand types -- the
    promise of ``TapLayer.invalidate``'s docstring, for the eval folds, the fp16 folded images and the padded biases as well as the weight
    images."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    def fold_f16():
        """The fp16 folded image of every strided layer, asked for as an fp16 program that does not fold its BatchNorm asks for it."""
        with torch.no_grad(), L.operand("f16"):
            for _, l in layers_of(model):
                if l.fold_geom() is not None:
                    l.packed_folded()

    widths, W, small = "c128", 128, True  # (the folded strided forms run here)
    model = build(widths)
    batch = batch_of(2, 16, W, 3)
    check_cold_rebuilds_agree(model, widths, batch, ("bf16", "f16"), small)
    _, o_before = check_warm(model, widths, batch, "bf16", small, label="6 first eval")
    check_warm(model, widths, batch, "f16", small, label="6 first eval")
    fold_f16()
    expect(audit(model), "packed", "packed_f16", "fold_f16", "eval_fold", "eval_fold_folded", "bias_pad")
    gen = torch.Generator().manual_seed(6)
    for name, p in list(model.named_parameters()) + list(model.named_buffers()):
        if not p.dtype.is_floating_point:
            continue
        v = p._version
        scale = 0.5 * float(p.detach().abs().mean())
        noise = torch.rand(p.shape, generator=gen)  # (zero-mean, except on the variances, which stay positive)
        p.data.add_((scale * (noise if "running_var" in name else 2.0 * noise - 1.0)).to(DEV))
        assert p._version == v, name  # (the premise: torch did not see it)
    E.invalidate_packed_weights(model)
    check_warm(model, widths, batch, "bf16", small, before=o_before, label="6 after invalidate")
    check_warm(model, widths, batch, "f16", small, label="6 after invalidate")
    fold_f16()
    expect(audit(model), "packed", "packed_f16", "fold_f16", "eval_fold", "eval_fold_folded", "bias_pad")


def test_deepcopy_of_a_warm_model():
    """7. ``copy.deepcopy`` of a warm model (EMA / SWA wrappers): the copy carries deep-copied ``_rv_layer`` objects that are not in
    ``engine._LAYERS``.  The original trains two more steps; then each equals the cold model of its own state.  The copy trains a step too."""
    from range_view_3d_detection_amd import engine as E

    model = build("c32")
    batch = batch_of(2, 16, 64, 3)
    check_cold_rebuilds_agree(model, "c32", batch)
    opt = optimiser(model)
    train(model, opt, [batch_of(2, 16, 64, 71)])
    _, o_first = check_warm(model, "c32", batch, label="7 warm")
    twin = copy.deepcopy(model)
    layers = [m.__dict__["_rv_layer"] for m in twin.modules() if "_rv_layer" in m.__dict__]
    assert len(layers) > 40 and not any(l in E._LAYERS for l in layers)
    train(model, opt, [batch_of(2, 16, 64, 72), batch_of(2, 16, 64, 73)])
    twin_out, o_twin = check_warm(twin, "c32", batch, label="7 copy")
    assert rel_err(o_twin[0], o_first[0]) == 0.0  # (the copy's state is the state at the time of the copy)
    expect(audit(twin), "packed", "eval_fold", "bias_pad")
    own, _ = check_warm(model, "c32", batch, before=o_first, label="7 original after two more steps")
    assert not torch.equal(own[0], twin_out[0])
    expect(audit(model), "packed", "eval_fold", "bias_pad")
    train(twin, optimiser(twin), [batch_of(2, 16, 64, 74)], between=lambda: expect(audit(twin), "packed"))
    check_warm(twin, "c32", batch, before=o_twin, label="7 copy after a step of its own")
    expect(audit(twin), "packed", "eval_fold", "bias_pad")


def _batched(model):
    """Layers of ``model`` whose served images are the persistent buffers ``prepack_stale`` writes."""
    held = [l.images.held(("weight", "gather", "bf16")) for _, l in layers_of(model)]  # (stale after the optimiser step: held, not current)
    return sum(1 for e in held if e is not None and e.persistent)


def test_prepack_stale_subsets():
    """8. ``prepack_stale``: exactly one stale layer (the ``< 2`` early return), a layer seen for the first time in the same step as stale
    ones, a second model trained in the same process (the device table of ``rv_pack_batch`` rebuilt), the first model deleted and a third of other widths
    trained.  The audit runs in every step, after backward: the images the step ran on are current then."""
    from range_view_3d_detection_amd import engine as E

    gc.collect()  # (``prepack_stale`` looks at every live layer of the process)

    def audited(model):
        return lambda: expect(audit(model), "packed", "bias_pad")

    a = build("c32")
    opt_a = optimiser(a)
    bs = [batch_of(2, 16, 64, s) for s in (81, 82, 83)]
    train(a, opt_a, bs[:2], between=audited(a))
    assert _batched(a) > 40  # (the second step ran on the batched re-pack)
    slot = ("weight", "gather", "bf16")
    buffers = {l: l.images.held(slot).data for _, l in layers_of(a) if l.images.held(slot).persistent}
    train(a, opt_a, bs[2:], between=audited(a))
    assert all(l.images.held(slot).data is buf for l, buf in buffers.items())  # (rewritten in place: the device table stays valid)
    # exactly one stale layer: every image is current after this forward/backward; then ONE weight changes
    a.train()
    a(bs[0]).backward()
    conv = _edit_targets(a)[0]
    with torch.no_grad():
        conv.weight.mul_(1.05)
    stale = [l for l in E._LAYERS if (held := [e.current for e in l.images.entries() if e.slot[0] == "weight"]) and not any(held)]
    assert len(stale) == 1 and stale[0].weight is conv.weight
    a(bs[1]).backward()
    counts = audit(a)
    assert counts["stale_skipped"] == 0, counts
    expect(counts, "packed", "bias_pad")
    # a layer seen for the first time together with stale ones
    opt_a.step()
    del conv.__dict__["_rv_layer"]
    train(a, opt_a, bs[:1], between=audited(a))
    assert audit(a)["stale_skipped"] > 40  # (after the optimiser step everything waits for its re-pack: the audit says so)
    # a second model in the same process, steps interleaved
    b = build("c32", seed=3)
    opt_b = optimiser(b)
    for i in range(3):
        train(b, opt_b, [bs[i]], between=audited(b))
        train(a, opt_a, [bs[i]], between=audited(a))
    assert _batched(a) > 40 and _batched(b) > 40
    batch = batch_of(2, 16, 64, 3)
    check_warm(b, "c32", batch, label="8 second model")
    # the first model gone, a third one of other widths
    del a, opt_a, conv, stale, audited, buffers
    gc.collect()
    c = build("c64", seed=4)
    opt_c = optimiser(c)
    for i in range(3):
        train(c, opt_c, [bs[i]], between=lambda: expect(audit(c), "packed", "bias_pad"))
        train(b, opt_b, [bs[i]], between=lambda: expect(audit(b), "packed", "bias_pad"))
    assert _batched(c) > 40
    check_warm(c, "c64", batch, label="8 third model")
    check_warm(b, "c32", batch, label="8 second model again")
    expect(audit(b), "packed", "eval_fold", "bias_pad")
    expect(audit(c), "packed", "eval_fold", "bias_pad")


def test_shape_changes_between_calls():
    """9. Train at 2 x 16 x 64, eval at 1 x 16 x 96, train at 1 x 16 x 64, eval at 2 x 16 x 64."""
    model = build("c32")
    wide, narrow = batch_of(1, 16, 96, 3), batch_of(2, 16, 64, 4)
    check_cold_rebuilds_agree(model, "c32", wide)
    check_cold_rebuilds_agree(model, "c32", narrow)
    o_wide, o_narrow = oracle_eval(state_of(model), wide), oracle_eval(state_of(model), narrow)
    opt = optimiser(model)
    train(model, opt, [batch_of(2, 16, 64, 91), batch_of(2, 16, 64, 92)])
    check_warm(model, "c32", wide, before=o_wide, label="9 eval 1x16x96")
    expect(audit(model), "packed", "eval_fold", "bias_pad")
    train(model, opt, [batch_of(1, 16, 64, 93), batch_of(1, 16, 64, 94)])
    check_warm(model, "c32", narrow, before=o_narrow, label="9 eval 2x16x64")
    expect(audit(model), "packed", "eval_fold", "bias_pad")


def test_range_partition_bounds_cache():
    """10. ``RangePartition``'s host copies of the band bounds: ``lower_bounds.copy_`` is picked up -- eval equals a cold
    rebuild of the same state at all four strides."""
    from range_view_3d_detection_amd.nn.backbones.dla import RangeNet

    def make():
        C = 32
        return RangeNet(in_channels=5, layers=[C] * 5, out_channels=C, projection_kernel_size=1, dataset_name="av2", num_neighbors=3, num_layers=2,
                        stem_type="RANGE_PARTITION", _net={"_target_": "torchbox3d.nn.backbones.dla.RangeBackbone", "in_channels": 5, "layers": [C] * 5, "out_channels": C})

    def run(net):
        net.eval()
        with torch.no_grad():
            out = net({k: batch[k] for k in ("features", "cart", "mask")})
        return {s: v.float().cpu() for s, v in out.items()}

    def rebuilt(net):
        fresh = make()
        fresh.load_state_dict(copy.deepcopy(state_of(net)))
        return fresh.to(DEV)

    torch.manual_seed(0)
    net = _randomise(make(), 1).to(DEV)
    batch = batch_of(2, 16, 64, 3)
    first, again = run(net), run(rebuilt(net))
    assert all(torch.equal(first[s], again[s]) for s in first)
    assert "_rv_bounds" in net.stem.__dict__
    with torch.no_grad():
        net.stem.lower_bounds.copy_(net.stem.lower_bounds + 7)  # (ranges of the synthetic sweep lie between 1.5 and 50: several bands change)
    moved, ref = run(net), run(rebuilt(net))
    assert not torch.equal(moved[1], first[1])
    for s in moved:
        assert torch.isfinite(moved[s]).all() and torch.equal(moved[s], ref[s]), s
    expect(audit(net), "eval_fold")  # (every conv of this backbone has a BatchNorm behind it: in eval mode there is no other image)


def test_batchnorm_tensors_swapped_through_data():
    """11. ``bn.weight.data`` / ``bn.bias.data`` / ``bn.running_var.data`` of every BatchNorm replaced, one attribute at a time, by a scaled
    clone (x 1.5, far above a bf16 ulp): no version counter moves and ``running_mean`` stays where it is -- only the swapped tensor's pointer
    tells.  Under both operand types the next eval differs from the one before the swap and equals a cold rebuild of the current state."""
    model = build("c32")
    batch = batch_of(2, 16, 64, 3)
    tags = ("bf16", "f16")
    check_cold_rebuilds_agree(model, "c32", batch, tags)
    last = {tag: evaluate(model, batch, tag) for tag in tags}
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) > 40
    for attr in ("weight", "bias", "running_var"):
        for bn in bns:
            t = getattr(bn, attr)
            version, mean_ptr = t._version, bn.running_mean.data_ptr()
            t.data = 1.5 * t.detach().clone()
            assert t._version == version and bn.running_mean.data_ptr() == mean_ptr, attr  # (the premise: no version moved)
        for tag in tags:
            warm = evaluate(model, batch, tag)
            ref = evaluate(cold(model, "c32"), batch, tag)
            assert not torch.equal(warm[0], last[tag][0]) and not torch.equal(warm[1], last[tag][1]), (attr, tag, "the old fold was served")
            assert torch.equal(warm[0], ref[0]) and torch.equal(warm[1], ref[1]), (attr, tag, rel_err(warm[0], ref[0]), rel_err(warm[1], ref[1]))
            last[tag] = warm
        expect(audit(model), "eval_fold", "bias_pad")
