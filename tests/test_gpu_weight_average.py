"""Weight averaging (EMA / SWA) in the fused AdamW launch, ``optim.AveragedModel`` and ``optim.update_bn``
(``rv_adamw_step_groups_avg`` / ``rv_average_tensors``, ``include/rv3d_optim.h``) against ``torch.optim.swa_utils`` and the oracle.

Shapes are the ``SIZES`` of ``test_gpu_optim_groups.py`` (they straddle the 65536-element chunk, the 4-wide vector and a single element); the
averaged twin of ``OFFSET`` is a view at element offset 1 of a larger buffer -- 4-byte but not 16-byte aligned --, so its chunk takes the
scalar path of ``a``.  Tolerances against torch are that file's: 2e-6 of a tensor's max-abs.

The learning rates of the trajectories are large (0.1 / 0.03: an Adam step moves an element by about its rate) on purpose: an average of
parameters that hardly move cannot tell a skipped update from a made one, and the teeth of the trajectory test ask exactly that."""

from __future__ import annotations

import copy
import gc

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import get_ema_multi_avg_fn

from test_gpu_forward import DEV
from test_gpu_optim_groups import MOMENTS, OFFSET, SIZES, _Census, _close

pytestmark = pytest.mark.gpu

STEP_CALLS = ("rv_adamw_step", "rv_adamw_step_groups", "rv_adamw_step_groups_avg")


# ---------------------------------------------------------------------------------------------
# 1. kernel level
# ---------------------------------------------------------------------------------------------
def _misaligned(t):
    """A copy of ``t`` that is a view at element offset 1 of a larger buffer."""
    buf = torch.zeros(t.numel() + 8, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _average_tables(avgs, srcs):
    from range_view_3d_detection_amd import _lib as L

    ce = int(L.load().rv_optim_chunk_elems())
    table = torch.tensor([[a.data_ptr(), p.data_ptr(), a.numel()] for a, p in zip(avgs, srcs)], dtype=torch.int64).to(DEV)
    chunks = [(i, c) for i, a in enumerate(avgs) for c in range((a.numel() + ce - 1) // ce)]
    return table, torch.tensor(chunks, dtype=torch.int32).to(DEV), len(chunks)


def _lerp64(a, p, w):
    """at::lerp's expression in float64 on the fp32 inputs, the weight rounded to fp32."""
    w = float(np.float32(w))
    a, p = a.double(), p.double()
    return a + w * (p - a) if w < 0.5 else p - (p - a) * (1.0 - w)


def test_average_tensors_single_update():
    """One ``rv_average_tensors`` call per weight in {1, 0.75, 0.1, 1/3} over independent ``randn`` tensors (|p - a| of order 1): element-wise
    |got - ref| <= 2**-21 max(|a|, |p|) (three fp32 roundings of quantities of at most 2 max(|a|, |p|), plus the rounding of w: derived,
    not measured); w = 1 stores p exactly; the reference with ``decay`` in place of ``1 - decay`` is off by more than 100 bounds; a
    weight outside [0, 1] or a null table writes nothing."""
    from range_view_3d_detection_amd import _lib as L

    gen = torch.Generator().manual_seed(0)
    a0 = [torch.randn(s, generator=gen).to(DEV) for s in SIZES]
    ps = [torch.randn(s, generator=gen).to(DEV) for s in SIZES]
    ps0 = [p.clone() for p in ps]
    worst = 0.0
    for w in (1.0, 0.75, 0.1, 1.0 / 3.0):
        avgs = [_misaligned(a) if i == OFFSET else a.clone() for i, a in enumerate(a0)]
        table, chunks, n_chunks = _average_tables(avgs, ps)
        L.call("rv_average_tensors", L.ptr(table), L.ptr(chunks), n_chunks, w, L.stream_ptr())
        torch.cuda.synchronize()
        for i, (got, a, p) in enumerate(zip(avgs, a0, ps)):
            ref = _lerp64(a, p, w)
            bound = 2.0 ** -21 * torch.maximum(a.abs(), p.abs()).double()
            err = (got.double() - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (w, i, float((err - bound).max()))
            if w == 1.0:
                assert torch.equal(got, p), i
            # teeth: decay where 1 - decay belongs
            wrong = _lerp64(a, p, 1.0 - w)
            assert float((wrong - ref).abs().max()) > 100.0 * float(bound.max()), (w, i)
            assert torch.equal(ps[i], ps0[i]) and not torch.equal(got, a), i
    print(f"rv_average_tensors: largest error / bound {worst:.3f}")
    # refusals: non-zero, a message, nothing written
    avgs = [a.clone() for a in a0]
    table, chunks, n_chunks = _average_tables(avgs, ps)
    for tab, w, word in ((table, -0.25, b"avg_weight"), (table, 1.25, b"avg_weight"), (None, 0.5, b"null")):
        rc = L.load().rv_average_tensors(L.ptr(tab), L.ptr(chunks), n_chunks, w, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and word in L.load().rv_last_error()
        assert all(torch.equal(x, y) for x, y in zip(avgs, a0))


# ---------------------------------------------------------------------------------------------
# a small module: the SIZES as parameters, and a BatchNorm for its buffers
# ---------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self, base):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(b.clone()) for b in base])
        self.bn = torch.nn.BatchNorm2d(8)


def _nets(gen, n=2):
    base = [torch.randn(s, generator=gen) for s in SIZES]
    return [_Net(base).to(DEV) for _ in range(n)]


def _groups(net, amsgrad=True):
    """A decay and a no-decay group with their own hyper-parameters, amsgrad on the second (which holds the misaligned tensors)."""
    params = list(net.parameters())
    return [{"params": [p for p in params if p.ndim >= 2], "lr": 0.1, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.05},
            {"params": [p for p in params if p.ndim <= 1], "lr": 0.03, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.0, "amsgrad": amsgrad}]


NO_GRAD_STEP, NO_GRAD_PARAM, CLIPPED_STEP = 3, 2, 2


def _step_inputs(gen, net, it):
    """Gradients (large on ``CLIPPED_STEP``; none for one parameter on ``NO_GRAD_STEP``) and buffer increments of step ``it``."""
    grads = [torch.randn(p.shape, generator=gen) * (5.0 if it == CLIPPED_STEP else 0.01) for p in net.parameters()]
    if it == NO_GRAD_STEP:
        grads[NO_GRAD_PARAM] = None
    return grads, [0.3 * torch.randn(8, generator=gen), 0.3 * torch.rand(8, generator=gen)]


def _install(net, grads, moves):
    """The gradients (the one of ``OFFSET`` a misaligned view) and the movement of the buffers a training forward would cause."""
    for i, (p, g) in enumerate(zip(net.parameters(), grads)):
        p.grad = None if g is None else _misaligned(g.to(DEV)) if i == OFFSET else g.clone().to(DEV)
    with torch.no_grad():
        net.bn.running_mean += moves[0].to(DEV)
        net.bn.running_var += moves[1].to(DEV)
        net.bn.num_batches_tracked += 3


def _misalign_twin(averaged):
    p = averaged.module.ps[OFFSET]
    p.data = _misaligned(p.data)


def test_fused_step_leaves_the_optimiser_alone():
    """Two identical optimisers (two groups, amsgrad on one, clipping active on one step, one parameter without a gradient on one step)
    through 5 steps, one fused with an EMA: parameters, every moment and ``last_grad_norm`` are ``torch.equal``; the fused run issues
    exactly one ``rv_adamw_step_groups_avg`` per step and nothing else of the family, the plain run exactly today's calls."""
    from range_view_3d_detection_amd.optim import AdamW, AveragedModel

    gen = torch.Generator().manual_seed(1)
    na, nb = _nets(gen)
    oa, ob = AdamW(_groups(na), max_grad_norm=35.0), AdamW(_groups(nb), max_grad_norm=35.0)
    ema = AveragedModel(na, decay=0.9)
    _misalign_twin(ema)
    ema.fuse(oa, na)
    fused_calls, plain_calls = [], []
    for it in range(5):
        grads, moves = _step_inputs(gen, na, it)
        _install(na, grads, moves)
        _install(nb, grads, moves)
        with _Census() as calls:
            oa.step()
            ema.update_parameters(na)
        fused_calls += calls
        with _Census() as calls:
            ob.step()
        plain_calls += calls
        assert torch.equal(oa.last_grad_norm, ob.last_grad_norm), it
        assert (float(ob.last_grad_norm) > 35.0) == (it == CLIPPED_STEP)
    assert [fused_calls.count(k) for k in STEP_CALLS] == [0, 0, 5], fused_calls
    assert [plain_calls.count(k) for k in STEP_CALLS] == [0, 5, 0] and plain_calls.count("rv_average_tensors") == 0, plain_calls
    assert fused_calls.count("rv_average_tensors") == 5 + 1  # the buffers every time; the parameter without a gradient once
    for i, (p, q) in enumerate(zip(na.parameters(), nb.parameters())):
        assert torch.equal(p.detach(), q.detach()), i
        sa, sb = oa.state[p], ob.state[q]
        assert set(sa) == set(sb) and float(sa["step"]) == float(sb["step"]) == (4.0 if i == NO_GRAD_PARAM else 5.0)
        for k in MOMENTS:
            if k in sb:
                assert torch.equal(sa[k], sb[k]), (i, k)
    assert any("max_exp_avg_sq" in oa.state[p] for p in na.parameters())
    # and the average is one: not the parameters, not its starting point
    assert all(not torch.equal(a, p) for a, p in zip(ema.module.parameters(), na.parameters()))
    assert int(ema.n_averaged) == 5 and all(not a.requires_grad for a in ema.module.parameters())


# ---------------------------------------------------------------------------------------------
# 3. trajectory against torch
# ---------------------------------------------------------------------------------------------
def _compare_averaged(ours, theirs, what):
    a, b = ours.state_dict(), theirs.state_dict()
    assert list(a) == list(b), what
    for k in a:
        x, y = a[k], b[k].to(a[k].device)
        if x.is_floating_point():
            _close(x, y, (what, k))
        else:
            assert torch.equal(x, y), (what, k, x, y)


@pytest.mark.parametrize("use_buffers", [False, True])
@pytest.mark.parametrize("decay", [0.9, None])
def test_trajectory_against_torch(decay, use_buffers):
    """The 5 steps of the test above: our fused ``AveragedModel`` against torch's, updated after a ``torch.optim.AdamW`` step (+
    ``clip_grad_norm_``) on identical clones.  Every averaged tensor within 2e-6 of its max-abs, ``n_averaged`` and the integer buffers equal.

    SWA with ``use_buffers=True``: torch's class cannot run that on a CUDA module that has a BatchNorm (``_foreach_addcdiv_`` refuses the
    integer ``num_batches_tracked``: "Integer division with addcdiv is no longer supported"), so torch's averaged copy lives on the CPU
    there, where the class applies ``get_swa_avg_fn`` -- averaged + (current - averaged) / (n + 1), truncated into the integer buffer --,
    which is the expression ours uses for integer buffers.

    Teeth (EMA, ``use_buffers=False``; on torch's side): an averaged copy that skips one update, and one that makes one twice, end more
    than 100 tolerances from the true one in some tensor."""
    from range_view_3d_detection_amd.optim import AdamW, AveragedModel

    gen = torch.Generator().manual_seed(2)
    na, nb = _nets(gen)
    oa, ob = AdamW(_groups(na), max_grad_norm=35.0), torch.optim.AdamW(_groups(nb))
    ours = AveragedModel(na, use_buffers=use_buffers, decay=decay)
    fn = None if decay is None else get_ema_multi_avg_fn(decay)
    theirs = torch.optim.swa_utils.AveragedModel(nb, device="cpu" if decay is None and use_buffers else None, multi_avg_fn=fn, use_buffers=use_buffers)
    teeth = decay is not None and not use_buffers
    skipped, twice = (torch.optim.swa_utils.AveragedModel(nb, multi_avg_fn=fn) for _ in range(2)) if teeth else (None, None)
    _misalign_twin(ours)
    ours.fuse(oa, na)
    for it in range(5):
        grads, moves = _step_inputs(gen, na, it)
        _install(na, grads, moves)
        _install(nb, grads, moves)
        torch.nn.utils.clip_grad_norm_(list(nb.parameters()), 35.0)
        oa.step()
        ours.update_parameters(na)
        ob.step()
        theirs.update_parameters(nb)
        if teeth:
            for m, times in ((skipped, 0 if it == 3 else 1), (twice, 2 if it == 3 else 1)):
                for _ in range(times):
                    m.update_parameters(nb)
        _compare_averaged(ours, theirs, (decay, use_buffers, it))
    assert int(ours.n_averaged) == 5 and ours.n_averaged.is_cuda
    assert int(ours.module.bn.num_batches_tracked) != int(na.bn.num_batches_tracked) or not use_buffers
    if teeth:
        ref = theirs.state_dict()
        for m in (skipped, twice):
            far = max(float((v - ref[k]).abs().max()) / (2e-6 * float(ref[k].abs().max())) for k, v in m.state_dict().items() if v.is_floating_point())
            assert far > 100.0, far


# ---------------------------------------------------------------------------------------------
# 4. protocol
# ---------------------------------------------------------------------------------------------
def test_protocol():
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.optim import AdamW, AveragedModel

    gen = torch.Generator().manual_seed(3)
    net, twin = _nets(gen)
    opt = AdamW(list(net.parameters()), lr=0.05, max_grad_norm=35.0)  # the shipped recipe: one group
    ema = AveragedModel(net, decay=0.9)
    theirs = torch.optim.swa_utils.AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(0.9))

    def inputs(it):
        grads, moves = _step_inputs(gen, net, it)
        _install(net, grads, moves)

    # never fused: today's call; update_parameters alone is a whole update equal to torch's
    for it in range(2):
        inputs(0)
        with _Census() as calls:
            opt.step()
            ema.update_parameters(net)
        theirs.update_parameters(net)
        assert [calls.count(k) for k in STEP_CALLS] == [1, 0, 0]
        assert calls.count("rv_average_tensors") == (1 if it == 0 else 2)  # a copy of everything; then the parameters (w) and the buffers (1)
        _compare_averaged(ours=ema, theirs=theirs, what=("standalone", it))
    # fused: one call of the averaging step even for one group
    ema.fuse(opt, net)
    inputs(0)
    with _Census() as calls:
        opt.step()
    assert [calls.count(k) for k in STEP_CALLS] == [0, 0, 1]
    # a second fused step without update_parameters: RvError before anything is launched, nothing written
    inputs(0)
    torch.cuda.synchronize()
    before = [t.detach().clone() for p in net.parameters() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
    before += [a.detach().clone() for a in ema.module.parameters()]
    steps = [float(opt.state[p]["step"]) for p in net.parameters()]
    with _Census() as calls:
        with pytest.raises(L.RvError, match="update_parameters"):
            opt.step()
    torch.cuda.synchronize()
    assert not any(k.startswith("rv_") for k in calls), calls
    after = [t.detach() for p in net.parameters() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])] + [a.detach() for a in ema.module.parameters()]
    assert all(torch.equal(x, y) for x, y in zip(before, after)) and steps == [float(opt.state[p]["step"]) for p in net.parameters()]
    with pytest.raises(L.RvError, match="update_parameters"):
        ema.unfuse()
    versions = [a._version for a in ema.module.parameters()]
    with _Census() as calls:
        ema.update_parameters(net)  # completes the pending step: buffers, count, version bumps
    theirs.update_parameters(net)
    assert calls.count("rv_average_tensors") == 1 and int(ema.n_averaged) == 3
    assert all(a._version > v for a, v in zip(ema.module.parameters(), versions))
    _compare_averaged(ema, theirs, "fused")
    # no step pending: a whole standalone update again
    inputs(0)
    opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.25)
    ema.update_parameters(net)
    theirs.update_parameters(net)
    _compare_averaged(ema, theirs, "standalone while fused")
    # unfuse: today's census
    ema.unfuse()
    inputs(0)
    with _Census() as calls:
        opt.step()
    assert [calls.count(k) for k in STEP_CALLS] == [1, 0, 0] and calls.count("rv_average_tensors") == 0
    # a custom averaging function is torch's path: nothing to fuse
    custom = AveragedModel(twin, avg_fn=lambda a, p, n: 0.5 * a + 0.5 * p)
    with pytest.raises(L.RvError, match="fuse"):
        custom.fuse(AdamW(list(twin.parameters())), twin)
    custom.update_parameters(twin)
    assert int(custom.n_averaged) == 1


# ---------------------------------------------------------------------------------------------
# 5. checkpoint interchange
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["torch_to_ours", "ours_to_torch"])
def test_checkpoint_interchange(direction):
    """Two SWA updates on one side, ``state_dict()`` into the other, one more update on both: they agree.  The weight of that update is
    1 / 3, which ours takes from the count mirror (refreshed from the loaded ``n_averaged``)."""
    from range_view_3d_detection_amd.optim import AveragedModel

    gen = torch.Generator().manual_seed(4)
    net, = _nets(gen, 1)
    ours, theirs = AveragedModel(net), torch.optim.swa_utils.AveragedModel(net)
    src, dst = (theirs, ours) if direction == "torch_to_ours" else (ours, theirs)

    def move():
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn(p.shape, generator=gen).to(DEV))
            net.bn.running_mean.add_(0.5)
            net.bn.num_batches_tracked.add_(1)

    for _ in range(2):
        move()
        src.update_parameters(net)
    dst.load_state_dict(copy.deepcopy(src.state_dict()))
    assert list(ours.state_dict()) == list(theirs.state_dict()) and int(dst.n_averaged) == 2
    assert all(torch.equal(x, y.to(x.device)) for x, y in zip(ours.state_dict().values(), theirs.state_dict().values()))
    assert all(not p.requires_grad for p in ours.module.parameters())
    move()
    ours.update_parameters(net)
    theirs.update_parameters(net)
    assert int(ours.n_averaged) == int(theirs.n_averaged) == 3
    _compare_averaged(ours, theirs, direction)
    # the weight was 1/3: the average is not the current parameters, and not the old average
    assert all(not torch.equal(a, p) for a, p in zip(ours.module.parameters(), net.parameters()))


# ---------------------------------------------------------------------------------------------
# 6. life cycle of the averaged module's cached images
# ---------------------------------------------------------------------------------------------
class _PackEntries:
    """``n_entries`` of every ``rv_pack_batch`` call issued inside the block."""

    def __enter__(self):
        from range_view_3d_detection_amd import _lib as L

        self.entries, self.real = [], L._call

        def spy(name, *args):
            if name == "rv_pack_batch":
                self.entries.append(int(args[1]))
            return self.real(name, *args)

        L._call = spy
        return self.entries

    def __exit__(self, *exc):
        from range_view_3d_detection_amd import _lib as L

        L._call = self.real


def test_life_cycle_of_the_averaged_module():
    """Train 2 fused steps, evaluate ``ema.module``, train 2 more: those steps did NOT re-pack the averaged module's layers (their
    cached images are stale, and the ``rv_pack_batch`` entry counts are those of a run without averaging); then ``ema.module``
    evaluates ``torch.equal`` to a cold rebuild from its state dict -- which a missing ``increment_version`` would break."""
    import test_gpu_lifecycle as LC
    from range_view_3d_detection_amd.optim import AveragedModel

    batches = [LC.batch_of(2, 16, 64, seed) for seed in (91, 92, 93, 94)]
    probe = LC.batch_of(2, 16, 64, 3)

    def run(averaging):
        gc.collect()  # (``prepack_stale`` looks at every live layer of the process)
        model = LC.build("c32")
        opt = LC.optimiser(model)
        ema, first = None, None
        if averaging:
            ema = AveragedModel(model, decay=0.9)
            ema.fuse(opt, model)
        with _PackEntries() as entries:
            for i, b in enumerate(batches):
                LC.train(model, opt, [b])
                if ema is not None:
                    ema.update_parameters(model)
                    if i == 1:
                        first = LC.evaluate(ema.module, probe)
        return model, ema, first, list(entries)

    model, _, _, plain_entries = run(False)
    del model
    model, ema, first, entries = run(True)
    assert entries == plain_entries and len(entries) >= 3 and min(entries) > 80, (entries, plain_entries)
    layers = [l for _, l in LC.layers_of(ema.module)]
    held = lambda kind: [(l, e) for l in layers for e in l.images.entries() if e.slot[0] == kind]
    # what the evaluation left behind: weight images of the convs without a BatchNorm, eval folds of the others -- all written twice
    # since by the fused step, none re-packed
    packed, folds = held("weight"), held("eval_fold")
    assert len({id(l) for l, _ in packed}) >= 2 and len(folds) > 40, (len(packed), len(folds))  # (``prepack_stale`` acts on two stale layers or more)
    assert not any(e.current for _, e in packed)
    assert all(e.sources[0] is l.weight and e.key[0] != (l.weight._version, l.weight.data_ptr()) for l, e in folds)  # (stale by the conv weight alone)
    assert all(not l.weight.requires_grad for l in layers)
    warm = LC.evaluate(ema.module, probe)
    ref = LC.evaluate(LC.cold(ema.module, "c32"), probe)
    assert torch.equal(warm[0], ref[0]) and torch.equal(warm[1], ref[1])
    assert not torch.equal(warm[0], first[0])  # the two steps in between moved the average
    own = LC.evaluate(model, probe)
    assert not torch.equal(own[0], warm[0])
    assert held("weight") and all(e.current for _, e in held("weight")) and {id(l) for l, _ in held("weight")} == {id(l) for l, _ in packed}
    assert len(held("eval_fold")) == len(folds) and all(e.current for _, e in held("eval_fold"))


# ---------------------------------------------------------------------------------------------
# 7. update_bn
# ---------------------------------------------------------------------------------------------
def test_update_bn_cumulative_average_vs_oracle(monkeypatch):
    """``optim.update_bn`` over three batches: every running statistic against the oracle stepping the same batches with its momentum
    1 / k for the k-th batch, within the bound of ``test_running_statistics_after_three_training_forwards_vs_oracle`` (1.5 x |fp32 oracle -
    bf16 oracle| + 1e-3 x max); ``num_batches_tracked == 3``; momenta and mode restored.  The same with ``torch.optim.swa_utils.update_bn``
    driving our model (``momentum=None``).  Control: momentum left at 0.1 differs from the cumulative result by more than three bounds
    in every tensor -- and without the engine's ``momentum is None`` rule the torch-driven run would equal this control."""
    import test_gpu_lifecycle as LC
    from oracle import model as om
    from range_view_3d_detection_amd import optim

    model = LC.build("c32")
    sd0 = LC.state_of(model)
    batches = [LC.batch_of(2, 16, 64, seed) for seed in (11, 12, 13)]
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]

    def stepped(make):
        sd = {k: (torch.zeros_like(v) if k.endswith("running_mean") else torch.ones_like(v) if k.endswith("running_var") else v) for k, v in sd0.items()}
        with torch.no_grad():
            for k, b in enumerate(batches, 1):
                monkeypatch.setattr(om, "BN_MOMENTUM", 1.0 / k)
                nm = make()
                om.detector_forward(b["features"].cpu(), b["cart"].cpu(), sd, nm=nm)
                assert nm.running
                sd.update(nm.running)
        monkeypatch.undo()
        return sd

    o32 = stepped(lambda: om.Numerics(train=True, running={}))
    o16 = stepped(lambda: om.Numerics.bf16(train=True))
    assert om.BN_MOMENTUM == 0.1
    keys = [k for k in sd0 if "running_" in k]
    bound = {k: 1.5 * float((o16[k].double() - o32[k].double()).abs().max()) + 1e-3 * float(o32[k].abs().max()) for k in keys}
    assert len(keys) == 2 * len(bns) and len(keys) > 100

    def check(label):
        got = LC.state_of(model)
        worst = (0.0, "")
        for k, v in got.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 3, (label, k)
        for k in keys:
            err = float((got[k].double() - o32[k].double()).abs().max())
            worst = max(worst, (err / bound[k], k))
            assert err <= bound[k], (label, k, err, bound[k])
        print(f"[{label}] {len(keys)} running statistics; largest error / bound {worst[0]:.3f} ({worst[1]})")
        return got

    for mode in (True, False):
        model.train(mode)
        bns[0].momentum, bns[1].momentum = 0.25, None
        optim.update_bn(batches if mode else [(b, "label") for b in batches], model)
        assert model.training is mode and bns[0].momentum == 0.25 and bns[1].momentum is None and all(m.momentum == 0.1 for m in bns[2:])
        bns[0].momentum = bns[1].momentum = 0.1
        ours = check(f"optim.update_bn, training={mode}")
    model.eval()
    torch.optim.swa_utils.update_bn(batches, model)
    assert not model.training and all(m.momentum == 0.1 for m in bns)
    check("torch.optim.swa_utils.update_bn")
    # control: three batches with the momentum left at 0.1
    for m in bns:
        m.reset_running_stats()
    model.train()
    with torch.no_grad():
        for b in batches:
            model(b)
    control = LC.state_of(model)
    far = sum(float((control[k].double() - ours[k].double()).abs().max()) > 3.0 * bound[k] for k in keys)
    print(f"[control] {far} of {len(keys)} running statistics more than 3 bounds from the cumulative average")
    assert far == len(keys), (far, len(keys))
