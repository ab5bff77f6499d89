"""The references of ``stem_ref.py`` against fp64 autograd: the positional pair and the modulation of the MetaKernel stem restated with
``F.unfold`` (the reference's nn/stems/__init__.py:64-85 -- ``oracle.model.meta_kernel`` wraps the projection and the fusion convs
around it, so its signature does not fit), training-mode BatchNorm, random fp64 data at 2 x 4 x 9 x 16.  Runs without a GPU."""

from __future__ import annotations

import torch
import torch.nn.functional as F

import bn_ref as R
import stem_ref as S

N, C, H, W = 2, 4, 9, 16
DIMS = (N, H, W)
EPS, MOM = 1e-5, 0.1
RTOL = 1e-10


def _close(got, want, what):
    scale = want.abs().max().clamp_min(1e-300)
    err = ((got - want).abs().max() / scale).item()
    assert err < RTOL, f"{what}: {err:.3e} of the maximum"


def _data():
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    # cart on a 2^-10 grid: the fp32 subtraction of `relative` is then exact, and the fp64 restatement forms the same numbers
    cart = (rnd(N, 3, H, W) * 4).mul(1024).round().div(1024)
    p = {"feat": rnd(N, C, H, W), "cart": cart, "w0": rnd(C, 3), "w1": rnd(C, C) * 0.5, "dgeo": rnd(N, C, 9, H * W)}
    for i in range(2):
        p[f"g{i}"], p[f"b{i}"] = 0.5 + torch.rand(C, generator=g, dtype=torch.float64), rnd(C) * 0.3
    return p


def _unfold_stem(p):
    """pos = MLP(rel) on the 9x grid, geo = pos * unfold(feat): (B, C, 9, H*W)."""
    fu = F.unfold(p["feat"], 3, padding=1).view(N, C, 9, H * W)
    nbr = F.unfold(p["cart"], 3, padding=1).view(N, 3, 9, H * W)
    pos = nbr - nbr[:, :, 4:5]
    for i in range(2):
        pos = F.conv2d(pos, p[f"w{i}"][:, :, None, None])
        pos = F.relu(F.batch_norm(pos, None, None, p[f"g{i}"], p[f"b{i}"], training=True, momentum=MOM, eps=EPS))
    return pos * fu


def _grid(t):
    """(B, C, 9, H*W) -> the kernels' 9x-grid layout (N*H*W*9, C)."""
    return t.permute(0, 3, 2, 1).reshape(N * H * W * 9, -1)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(N * H * W, -1)


def test_references_match_autograd_of_the_unfold_restatement():
    p = _data()
    leaves = ["feat", "w0", "w1", "g0", "b0", "g1", "b1"]
    for k in leaves:
        p[k].requires_grad_(True)
    geo_t = _unfold_stem(p)
    grads = dict(zip(leaves, torch.autograd.grad(geo_t, [p[k] for k in leaves], p["dgeo"])))
    q = {k: v.detach() for k, v in p.items()}
    feat, dgeo = _nhwc(q["feat"]), _grid(q["dgeo"]).reshape(N * H * W, 9 * C)

    # forward through the references
    rel = S.relative(q["cart"].float(), dtype=torch.float64)
    st1 = S.smallk_stats(rel, q["w0"], 3, q["g0"], q["b0"], EPS, MOM)
    h1, y2, ysum, ysq = S.pos_forward(rel, q["w0"], 3, st1["scale"], st1["shift"], q["w1"], dtype=torch.float64)
    assert torch.equal(h1, S.smallk_apply(rel, q["w0"], 3, st1["scale"], st1["shift"], True))
    st2 = R.bn_finalize(y2, q["g1"], q["b1"], EPS, MOM)
    n9 = y2.shape[0]
    _close(ysum / n9, st2["mean"], "pos_forward sum")
    _close(ysq / n9 - (ysum / n9) ** 2, y2.var(0, unbiased=False), "pos_forward sum of squares")
    geo = S.modulate(y2, st2["scale"], st2["shift"], feat, DIMS)
    _close(geo, _grid(geo_t.detach()).reshape(N * H * W, 9 * C), "forward")
    _close(S.pos_modulate(rel, q["w0"], 3, st1["scale"], st1["shift"], q["w1"], st2["scale"], st2["shift"], feat, DIMS, dtype=torch.float64), geo, "pos_modulate")

    # backward: modulation + second BatchNorm
    s0, s1, dfeat = S.modulate_bwd_sums(dgeo, y2, st2["scale"], st2["shift"], st2["mean"], st2["invstd"], feat, DIMS)
    _close(dfeat, _nhwc(grads["feat"]), "dfeat")
    dpos_act, dfeat_u = S.modulate_bwd(dgeo, y2, st2["scale"], st2["shift"], feat, DIMS)
    assert torch.equal(dfeat_u, dfeat)
    z = R.masked_grad(dpos_act, None, y2, st2["scale"], st2["shift"], True)
    assert torch.equal(z, S.modulate_z(dgeo, y2, st2["scale"], st2["shift"], feat, DIMS))
    _close(s1, grads["g1"], "dgamma of the second layer")
    _close(s0, grads["b1"], "dbeta of the second layer")
    coef = R.bwd_finalize(s0, s1, n9, q["g1"], st2["invstd"])[2]
    dy2 = S.modulate_bwd_apply(dgeo, y2, st2["scale"], st2["shift"], st2["mean"], st2["invstd"], coef, feat, DIMS)
    _close(dy2.t() @ h1, grads["w1"], "dW of the second layer")

    # backward: first layer (its input needs no gradient)
    w2s = q["w1"].t().contiguous()  # the scatter image [ci][co]
    g, y1 = S.pos_masked_grad(dy2, w2s, rel, q["w0"], 3, st1["scale"], st1["shift"])
    p0, p1, pr = S.pos_backward_planes(dy2, w2s, rel, q["w0"], 3, st1["scale"], st1["shift"], st1["mean"], st1["invstd"])
    dgamma, dbeta, dw = S.smallk_grads(g, y1, rel, 3, q["g0"], st1["mean"], st1["invstd"])
    assert torch.equal(p1, dgamma) and torch.equal(p0, dbeta)
    _close(dgamma, grads["g0"], "dgamma of the first layer")
    _close(dbeta, grads["b0"], "dbeta of the first layer")
    _close(dw, grads["w0"], "dW of the first layer")
    # ... and the generic small-K planes on the same layer: dOut = dh1 (ungated), y recomputed from the input.  dh1 is formed from the
    # scatter image, as pos_masked_grad forms it: the same product through another operand layout may round differently (it does on
    # some CPUs), and the comparisons with `g` below are exact
    dh1 = dy2 @ w2s.t()
    k0, k1, kr, kg = S.smallk_bwd_planes(dh1, None, None, rel, q["w0"], 3, 4, st1["scale"], st1["shift"], st1["mean"], st1["invstd"],
                                         S.BNB_Y_FROM_INPUT | S.BNB_RELU_Z)
    assert torch.equal(kg, g)
    _close(k0, p0, "small-K S0")
    _close(k1, p1, "small-K S1")
    _close(kr[:3], pr, "small-K R")
    # the stored-y form: y = the raw output, the `out` mask = the activated output
    act = S.smallk_apply(rel, q["w0"], 3, st1["scale"], st1["shift"], True)
    m0, m1, mr, mg = S.smallk_bwd_planes(dh1, act, y1, rel, q["w0"], 3, 4, st1["scale"], st1["shift"], st1["mean"], st1["invstd"], 0)
    assert torch.equal(mg, g)
    # the moments identity the kernels use, against the definition
    m1v, m2v = S.smallk_moments(rel, 4)
    wv = q["w0"]
    _close(wv @ m1v[:3] / n9, st1["mean"], "mean from the moments")
    _close(((wv @ m2v[:3, :3]) * wv).sum(1) / n9 - st1["mean"] ** 2, y1.var(0, unbiased=False), "variance from the moments")


def test_smallk_grads_with_global_sums():
    """SyncBN: two ranks with the same data -- global sums twice the local ones, twice the count -- give the single-rank gradients."""
    g_ = torch.Generator().manual_seed(3)
    v = torch.randn(50, 8, generator=g_, dtype=torch.float64)
    w = torch.randn(6, 8, generator=g_, dtype=torch.float64)
    g = torch.randn(50, 6, generator=g_, dtype=torch.float64)
    gamma = torch.rand(6, generator=g_, dtype=torch.float64) + 0.5
    y = S.smallk_y(v, w, 5)
    mean, invstd = y.mean(0), 1.0 / torch.sqrt(y.var(0, unbiased=False) + EPS)
    dgamma, dbeta, dw = S.smallk_grads(g, y, v, 5, gamma, mean, invstd)
    d2 = S.smallk_grads(g, y, v, 5, gamma, mean, invstd, global_s01=torch.stack([2 * dbeta, 2 * dgamma]), count=100)
    _close(d2[2], dw, "dW under SyncBN")
    # against autograd of the conv + BatchNorm
    wl = w[:, :5].clone().requires_grad_(True)
    out = F.batch_norm((v[:, :5] @ wl.t()), None, None, gamma, torch.zeros(6, dtype=torch.float64), training=True, eps=EPS)
    (gw,) = torch.autograd.grad(out, wl, g)
    _close(dw, gw, "dW")


def test_relative_tap_order_and_orientation():
    """Hand-written 1 x 3 x 2 x 3 cart: tap k = 3 ky + kx is the neighbour (h + ky - 1, w + kx - 1); outside the image it is -centre."""
    cart = torch.zeros(1, 3, 2, 3)
    for j in range(3):
        for h in range(2):
            for w in range(3):
                cart[0, j, h, w] = 100 * (j + 1) + 10 * h + w
    rel = S.relative(cart, dtype=torch.float32).reshape(2, 3, 9, 32)
    assert bool((rel[..., 3:] == 0).all())
    for h in range(2):
        for w in range(3):
            for ky in range(3):
                for kx in range(3):
                    hn, wn = h + ky - 1, w + kx - 1
                    inside = 0 <= hn < 2 and 0 <= wn < 3
                    for j in range(3):
                        want = (float(cart[0, j, hn, wn]) if inside else 0.0) - float(cart[0, j, h, w])
                        assert rel[h, w, 3 * ky + kx, j].item() == want, (h, w, ky, kx, j)
    # spot values: pixel (0, 1): tap 5 = (0, 2) is one column to the right, tap 7 = (1, 1) one row below, tap 1 = (-1, 1) outside
    assert rel[0, 1, 5, 0].item() == 1.0 and rel[0, 1, 7, 0].item() == 10.0 and rel[0, 1, 1, 0].item() == -101.0 and rel[0, 1, 4, 2].item() == 0.0
    # the gathers share the orientation: feature of the neighbour, and the adjoint puts it back
    x = torch.arange(6, dtype=torch.float64).reshape(6, 1) + 1
    g9 = S.gather9(x, (1, 2, 3))
    assert g9[1, 5, 0].item() == 3.0 and g9[1, 7, 0].item() == 5.0 and g9[1, 1, 0].item() == 0.0
    t = torch.randn(6, 9, 1, dtype=torch.float64)
    assert abs(float((S.scatter9(t, (1, 2, 3)) * x).sum() - (t * g9).sum())) < 1e-12
