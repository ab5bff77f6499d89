"""``optim.AdamW`` beyond the shipped recipe -- several parameter groups under ONE clipping norm, per-parameter step counts, amsgrad,
maximize, checkpoint interchange (``rv_adamw_step_groups``, ``include/rv3d_optim.h``) -- against ``torch.optim.AdamW`` (its default
foreach path) + ``torch.nn.utils.clip_grad_norm_`` on identical clones.

Tolerances are those of ``test_gpu_model.py::test_fused_adamw_matches_torch_adamw_with_clipping``: parameters and every moment within
2e-6 of that tensor's max-abs, the reported norm within 1e-6 relative.  The sizes are that test's (they straddle the 65536-element
chunk, the 4-wide vector and a single element) plus one parameter whose gradient is a view at element offset 1 of a larger buffer:
4-byte but not 16-byte aligned, so its chunk takes the scalar path of the kernel."""

from __future__ import annotations

import copy

import pytest
import torch

from test_gpu_forward import DEV

pytestmark = pytest.mark.gpu

SIZES = [(1,), (3,), (7, 11), (1000,), (65536 + 5,), (3, 70001), (256, 256, 3, 3), (1001,)]
OFFSET = len(SIZES) - 1  # the parameter whose gradient is not 16-byte aligned
DECAY = [i for i, s in enumerate(SIZES) if len(s) >= 2]
NO_DECAY = [i for i, s in enumerate(SIZES) if len(s) <= 1]
MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _pair(gen, sizes=SIZES):
    base = [torch.randn(s, generator=gen) for s in sizes]
    return [torch.nn.Parameter(b.clone().to(DEV)) for b in base], [torch.nn.Parameter(b.clone().to(DEV)) for b in base]


def _install(a, b, grads):
    """The same gradients on both copies (``None`` = no gradient); on the fused side the one of ``OFFSET`` is a misaligned view."""
    for i, (p, q, g) in enumerate(zip(a, b, grads)):
        if g is None:
            p.grad = q.grad = None
            continue
        q.grad = g.clone().to(DEV)
        if i == OFFSET:
            buf = torch.zeros(g.numel() + 8, device=DEV)
            view = buf[1:1 + g.numel()].view(g.shape)
            view.copy_(g)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            p.grad = view
        else:
            p.grad = g.clone().to(DEV)


def _grads(gen, scale, sizes=SIZES):
    return [torch.randn(s, generator=gen) * scale for s in sizes]


def _close(x, y, what):
    err = float((x.detach() - y.detach()).abs().max())
    bound = 2e-6 * max(float(y.detach().abs().max()), 1e-30)
    assert err <= bound, (what, err, bound)


def _compare(oa, ob, a, b, what=""):
    """Parameters, every moment and the step count of every parameter; the state of the two has the same keys (none without a gradient so far)."""
    for i, (p, q) in enumerate(zip(a, b)):
        _close(p, q, (what, i, "param"))
        sa, sb = oa.state.get(p, {}), ob.state.get(q, {})
        assert set(sa) == set(sb), (what, i, set(sa), set(sb))
        for k in MOMENTS:
            if k in sb:
                assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape and sa[k].stride() == sb[k].stride() and sa[k].device == sb[k].device
                _close(sa[k], sb[k], (what, i, k))
        if sb:
            assert not sa["step"].is_cuda and sa["step"].dtype == sb["step"].dtype and float(sa["step"]) == float(sb["step"]), (what, i)


def _norm_ok(oa, want):
    assert abs(float(oa.last_grad_norm) - float(want)) <= 1e-6 * float(want), (float(oa.last_grad_norm), float(want))


class _Census:
    """Names of the library calls issued inside the block (the call log ``test_gpu_model.py`` uses: ``_lib._call``)."""

    def __enter__(self):
        from range_view_3d_detection_amd import _lib as L

        self.calls, self.real = [], L._call

        def spy(name, *args):
            self.calls.append(name)
            return self.real(name, *args)

        L._call = spy
        return self.calls

    def __exit__(self, *exc):
        from range_view_3d_detection_amd import _lib as L

        L._call = self.real


def _two_groups(params, **second):
    """A decay and a no-decay group with their own hyper-parameters; ``second``: further keys of the second group's dict (it holds the
    misaligned gradient and a tensor of two chunks)."""
    return [{"params": [params[i] for i in DECAY], "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.05},
            {"params": [params[i] for i in NO_DECAY], "lr": 3e-4, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.0, **second}]


def test_two_groups_clipped_scheduled():
    """A decay and a no-decay group with their own lr / betas / eps / weight_decay under ``max_grad_norm=35`` and a ``OneCycleLR`` with
    one ``max_lr`` per group: one norm over both groups (active on step 2 only), one ``rv_adamw_step_groups`` call per step."""
    from range_view_3d_detection_amd.optim import AdamW

    gen = torch.Generator().manual_seed(0)
    a, b = _pair(gen)
    oa, ob = AdamW(_two_groups(a), max_grad_norm=35.0), torch.optim.AdamW(_two_groups(b))
    sa = torch.optim.lr_scheduler.OneCycleLR(oa, max_lr=[0.0015, 0.0006], total_steps=20)
    sb = torch.optim.lr_scheduler.OneCycleLR(ob, max_lr=[0.0015, 0.0006], total_steps=20)
    with _Census() as calls:
        for it in range(5):
            _install(a, b, _grads(gen, 5.0 if it == 2 else 0.01))
            want = torch.nn.utils.clip_grad_norm_(b, 35.0)
            oa.step()
            ob.step()
            sa.step()
            sb.step()
            _norm_ok(oa, want)
            assert (float(want) > 35.0) == (it == 2)
            for ga, gb in zip(oa.param_groups, ob.param_groups):
                assert ga["lr"] == gb["lr"] and ga["betas"] == gb["betas"] and ga["weight_decay"] == gb["weight_decay"] and ga["eps"] == gb["eps"]
    assert calls.count("rv_adamw_step_groups") == 5 and calls.count("rv_adamw_step") == 0
    assert oa.param_groups[0]["lr"] != oa.param_groups[1]["lr"] and oa.param_groups[0]["betas"][1] != oa.param_groups[1]["betas"][1]
    _compare(oa, ob, a, b)
    assert all(float(oa.state[p]["step"]) == 5.0 for p in a)


def test_per_parameter_step_counts():
    """One group; two tensors (one of several chunks) get their first gradient on step 2, a third has none on step 3, a fourth never
    has one: every parameter is bias-corrected with its own count, a parameter without a gradient keeps its step (or its empty state)."""
    from range_view_3d_detection_amd.optim import AdamW

    gen = torch.Generator().manual_seed(1)
    sizes = SIZES + [(5,)]  # the last one never receives a gradient
    late, skip3, never = (3, 5), 2, len(sizes) - 1
    assert SIZES[5] == (3, 70001)
    a, b = _pair(gen, sizes)
    oa, ob = AdamW(a, lr=1e-3, max_grad_norm=35.0), torch.optim.AdamW(b, lr=1e-3)
    for it in range(5):
        grads = _grads(gen, 5.0 if it == 2 else 0.01, sizes)
        for i in range(len(sizes)):
            if (i in late and it < 2) or (i == skip3 and it == 3) or i == never:
                grads[i] = None
        _install(a, b, grads)
        want = torch.nn.utils.clip_grad_norm_(b, 35.0)
        oa.step()
        ob.step()
        _norm_ok(oa, want)
        _compare(oa, ob, a, b, f"step {it}")
        for i, p in enumerate(a):
            if i == never:
                assert len(oa.state.get(p, {})) == 0
            elif i in late:
                assert it < 2 and len(oa.state.get(p, {})) == 0 or float(oa.state[p]["step"]) == it - 1
            elif i == skip3:
                assert float(oa.state[p]["step"]) == (it + 1 if it < 3 else it)
            else:
                assert float(oa.state[p]["step"]) == it + 1


def test_amsgrad_on_one_group():
    """amsgrad through the group dict of one of two groups: ``max_exp_avg_sq`` (torch's key, dtype and layout) follows torch's through a
    large-gradient step and three small ones, after which it exceeds ``exp_avg_sq``; the other group's state has no such key."""
    from range_view_3d_detection_amd.optim import AdamW

    gen = torch.Generator().manual_seed(2)
    a, b = _pair(gen)
    oa, ob = AdamW(_two_groups(a, amsgrad=True), lr=1e-3), torch.optim.AdamW(_two_groups(b, amsgrad=True), lr=1e-3)
    assert oa.param_groups[0]["amsgrad"] is False and oa.param_groups[1]["amsgrad"] is True
    for it in range(4):
        _install(a, b, _grads(gen, 100.0 if it == 0 else 0.01))
        oa.step()
        ob.step()
    for i in NO_DECAY:  # the precondition, on torch's side: the maximum is what the denominator took on every step after the first
        st = ob.state[b[i]]
        assert bool((st["max_exp_avg_sq"] >= st["exp_avg_sq"]).all()) and float((st["max_exp_avg_sq"] > st["exp_avg_sq"]).float().mean()) > 0.99
        assert set(oa.state[a[i]]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    for i in DECAY:
        assert set(oa.state[a[i]]) == {"step", "exp_avg", "exp_avg_sq"}
    _compare(oa, ob, a, b)


def test_maximize_with_clipping():
    from range_view_3d_detection_amd.optim import AdamW

    gen = torch.Generator().manual_seed(3)
    a, b = _pair(gen)
    oa, ob = AdamW(a, lr=1e-3, maximize=True, max_grad_norm=35.0), torch.optim.AdamW(b, lr=1e-3, maximize=True)
    before = [p.detach().clone() for p in a]
    for it in range(3):
        grads = _grads(gen, 5.0 if it == 1 else 0.01)
        _install(a, b, grads)
        want = torch.nn.utils.clip_grad_norm_(b, 35.0)
        oa.step()
        ob.step()
        _norm_ok(oa, want)
        assert (float(want) > 35.0) == (it == 1)
        if it == 0:
            # ascent: the first step moves an element by lr along the sign of its gradient, against a decay of 1e-5 |p|; only where
            # |g| comes near eps = 1e-8 (a handful of the 590k elements) is the step smaller than that, so those are left out
            g6 = grads[6].to(DEV)
            sure = g6.abs() > 1e-5
            assert int(sure.sum()) > 0.99 * g6.numel() and bool((((a[6].detach() - before[6]) * g6)[sure] > 0).all())
    _compare(oa, ob, a, b)


def _tables(ps, ms, vs, gs):
    """The device tables of ``rv_adamw_step`` / ``rv_adamw_step_groups`` for these tensors, as ``optim.AdamW`` builds them."""
    from range_view_3d_detection_amd import _lib as L

    ce = int(L.load().rv_optim_chunk_elems())
    tens = torch.tensor([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, g, m, v in zip(ps, gs, ms, vs)], dtype=torch.int64)
    chunks = [(i, c) for i, p in enumerate(ps) for c in range((p.numel() + ce - 1) // ce)]
    return {"tens": tens.to(DEV), "chunks": torch.tensor(chunks, dtype=torch.int32).to(DEV), "n_chunks": len(chunks),
            "partial": torch.empty(len(chunks), dtype=torch.float32, device=DEV), "row": torch.zeros(len(ps), dtype=torch.int32, device=DEV),
            "norm": torch.zeros(1, dtype=torch.float32, device=DEV)}


def test_common_case_unchanged():
    """One group with nothing special stays on ``rv_adamw_step`` (the call census), and ``rv_adamw_step_groups`` with one row computes
    the same parameters and moments bit for bit: the two kernels share the element function."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.optim import AdamW

    gen = torch.Generator().manual_seed(4)
    a, b = _pair(gen)
    oa = AdamW(a, lr=1e-3, max_grad_norm=35.0)
    ps = [q.detach() for q in b]
    ms, vs = [torch.zeros_like(q) for q in ps], [torch.zeros_like(q) for q in ps]
    worst = 0
    with _Census() as calls:
        for it in range(3):
            _install(a, b, _grads(gen, 5.0 if it == 1 else 0.01))
            oa.step()
            gs = [p.grad if i == OFFSET else q.grad for i, (p, q) in enumerate(zip(a, b))]  # (the misaligned view itself for OFFSET)
            t = _tables(ps, ms, vs, gs)
            rows = (L.AdamRow * 1)(L.AdamRow(1e-3, 0.9, 0.999, 1e-8, 1e-2, it + 1, 0))
            L.call("rv_adamw_step_groups", L.ptr(t["tens"]), L.ptr(t["row"]), None, L.ptr(t["chunks"]), t["n_chunks"], L.ptr(t["partial"]), rows, 1,
                   35.0, L.ptr(t["norm"]), L.stream_ptr())
            torch.cuda.synchronize()
            assert float(t["norm"]) == float(oa.last_grad_norm)
            for i, p in enumerate(a):
                for x, y in ((p.detach(), ps[i]), (oa.state[p]["exp_avg"], ms[i]), (oa.state[p]["exp_avg_sq"], vs[i])):
                    worst = max(worst, int((x.view(torch.int32).long() - y.view(torch.int32).long()).abs().max()))
    print(f"rv_adamw_step vs rv_adamw_step_groups with one row: largest difference {worst} ulp")
    assert calls.count("rv_adamw_step") == 3 and calls.count("rv_adamw_step_groups") == 3  # (the three direct calls of this test)
    for i, p in enumerate(a):
        assert torch.equal(p.detach(), ps[i]) and torch.equal(oa.state[p]["exp_avg"], ms[i]) and torch.equal(oa.state[p]["exp_avg_sq"], vs[i]), i
    # the optimiser alone: no grouped call for the one-group recipe; exactly one, and no rv_adamw_step, per step with two groups
    with _Census() as calls:
        _install(a, b, _grads(gen, 0.01))
        oa.step()
    assert calls.count("rv_adamw_step") == 1 and calls.count("rv_adamw_step_groups") == 0
    og = AdamW(_two_groups(a), max_grad_norm=35.0)
    with _Census() as calls:
        for _ in range(2):
            og.step()
    assert calls.count("rv_adamw_step_groups") == 2 and calls.count("rv_adamw_step") == 0


@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_checkpoint_interchange(direction):
    """Two steps of one optimiser (two groups, amsgrad on one), ``state_dict()`` into the other over cloned parameters, two more steps
    of both: the loaded optimiser continues as the one that wrote the checkpoint.

    The gradients are large (clip active) on ONE step, as in every test of this file and in the test the tolerances come from.  Two clipped
    steps were measured to miss the bound on the one-element tensor without anything being wrong: the two norms may differ by 1e-6
    relative (here ~1e-7), so may the two clip coefficients, and when two clipped gradients of opposite sign nearly cancel in ``exp_avg``
    (4e-3 - 4e-3 -> 1.2e-4) that 1e-7 of the terms is 3e-6 of the sum -- and a tensor of one element has no larger element to be measured against."""
    from range_view_3d_detection_amd.optim import AdamW

    gen = torch.Generator().manual_seed(5)
    a, b = _pair(gen)  # a: the fused optimiser's, b: torch's
    oa, ob = AdamW(_two_groups(a, amsgrad=True), max_grad_norm=35.0), torch.optim.AdamW(_two_groups(b, amsgrad=True))

    def step_both(scale):
        _install(a, b, _grads(gen, scale))
        want = torch.nn.utils.clip_grad_norm_(b, 35.0)
        oa.step()
        ob.step()
        _norm_ok(oa, want)

    src_opt, src, dst_opt, dst = (ob, b, oa, a) if direction == "torch_to_fused" else (oa, a, ob, b)
    for scale in (0.01, 5.0):  # (the destination steps along and is overwritten: only the source's state survives the load)
        step_both(scale)
    with torch.no_grad():
        for p, q in zip(dst, src):
            p.copy_(q)
    # (the deep copy stands for the trip through a file: state_dict() hands out the live tensors and load_state_dict() keeps them as they are)
    dst_opt.load_state_dict(copy.deepcopy(src_opt.state_dict()))
    for ga, gb in zip(oa.param_groups, ob.param_groups):
        assert all(ga[k] == gb[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"))
    for p, q in zip(dst, src):
        assert all(torch.equal(dst_opt.state[p][k], src_opt.state[q][k]) for k in src_opt.state[q])
        assert not dst_opt.state[p]["step"].is_cuda and dst_opt.state[p]["exp_avg"].data_ptr() != src_opt.state[q]["exp_avg"].data_ptr()
    for scale in (0.01, 0.01):
        step_both(scale)
    _compare(oa, ob, a, b, direction)
    assert all(float(oa.state[p]["step"]) == 4.0 for p in a)


def test_refusals():
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.optim import AdamW

    one = [torch.nn.Parameter(torch.ones(1, device=DEV))]
    for kw in ("capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=kw):
            AdamW(one, **{kw: True})
    # more distinct (group, step count) rows in one step than the kernel's arguments hold
    cap = int(L.load().rv_adam_max_rows())
    ps = [torch.nn.Parameter(torch.ones(1, device=DEV)) for _ in range(cap + 1)]
    for p in ps:
        p.grad = torch.ones(1, device=DEV)
    opt = AdamW([{"params": [p], "lr": 1e-3 * (1 + i)} for i, p in enumerate(ps)])
    with pytest.raises(L.RvError, match=r"rv_adam_max_rows\(\) = %d" % cap):
        opt.step()
    torch.cuda.synchronize()
    assert all(float(p.detach()) == 1.0 for p in ps) and all(float(opt.state[p]["step"]) == 0.0 for p in ps)
    AdamW([{"params": [p], "lr": 1e-3 * (1 + i)} for i, p in enumerate(ps[:cap])]).step()  # exactly the cap is fine
    torch.cuda.synchronize()
    assert all(float(p.detach()) < 1.0 for p in ps[:cap]) and float(ps[cap].detach()) == 1.0
    # n_rows = 0: non-zero with a message, nothing launched
    p, g, m, v = (torch.full((1000,), x, device=DEV) for x in (1.0, 0.5, 0.0, 0.0))
    t = _tables([p], [m], [v], [g])
    t["norm"].fill_(-1.0)
    rows = (L.AdamRow * 1)(L.AdamRow(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0))
    rc = L.load().rv_adamw_step_groups(L.ptr(t["tens"]), L.ptr(t["row"]), None, L.ptr(t["chunks"]), t["n_chunks"], L.ptr(t["partial"]), rows, 0, 35.0,
                                       L.ptr(t["norm"]), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"n_rows = 0" in L.load().rv_last_error()
    assert float(t["norm"]) == -1.0 and bool((p == 1.0).all()) and bool((m == 0.0).all()) and bool((v == 0.0).all())


def test_model_level_no_weight_decay_1d(golden):
    """The tiny model's own gradients (one HIP forward + backward) through ``configure_optimizers(no_weight_decay_1d=True)``: the fused form
    with the folded clipping against ``torch.optim.AdamW`` + ``clip_grad_norm_`` over the same two groups, three scheduled steps."""
    from range_view_3d_detection_amd.nn.meta.arch import configure_optimizers
    from test_gpu_model import load_tiny

    g = golden("tiny_model")
    backbone, head = load_tiny(g)
    backbone.train()
    head.train()
    data = {"features": g["features"].to(DEV), "cart": g["cart"].to(DEV), "mask": g["mask"].to(DEV), "annotations": g["annotations"]}
    _, losses = head(backbone(data), data, return_loss=True)
    losses["loss"].backward()
    named = [(f"backbone.{k}", p) for k, p in backbone.named_parameters()] + [(f"head.{k}", p) for k, p in head.named_parameters()]
    grads = [None if p.grad is None else p.grad.detach().clone() for _, p in named]
    assert sum(x is not None for x in grads) > 40 and all(torch.isfinite(x).all() for x in grads if x is not None)
    twins = [(k, torch.nn.Parameter(p.detach().clone())) for k, p in named]
    oa, sa = configure_optimizers(named, num_devices=1, batch_size=2, total_steps=10, no_weight_decay_1d=True, max_grad_norm=35.0, fused=True)
    ob, sb = configure_optimizers(twins, num_devices=1, batch_size=2, total_steps=10, no_weight_decay_1d=True, fused=False)
    assert isinstance(ob, torch.optim.AdamW) and not isinstance(oa, torch.optim.AdamW)
    for opt, pairs in ((oa, named), (ob, twins)):
        assert len(opt.param_groups) == 2 and opt.param_groups[0]["weight_decay"] == 1e-2 and opt.param_groups[1]["weight_decay"] == 0.0
        assert {id(p) for p in opt.param_groups[1]["params"]} == {id(p) for _, p in pairs if p.ndim <= 1}
        assert {id(p) for p in opt.param_groups[0]["params"]} == {id(p) for _, p in pairs if p.ndim >= 2}
    assert len(oa.param_groups[1]["params"]) > 10 and len(oa.param_groups[0]["params"]) > 10
    with _Census() as calls:
        for _ in range(3):
            for (_, p), (_, q), x in zip(named, twins, grads):
                p.grad = None if x is None else x.clone()
                q.grad = None if x is None else x.clone()
            want = torch.nn.utils.clip_grad_norm_([q for _, q in twins], 35.0)
            oa.step()
            ob.step()
            sa.step()
            sb.step()
            _norm_ok(oa, want)
    assert calls.count("rv_adamw_step_groups") == 3 and calls.count("rv_adamw_step") == 0
    for (k, p), (_, q) in zip(named, twins):
        _close(p, q, k)
