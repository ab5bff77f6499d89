"""``fused_bnb_ref.py`` (the fp64 restatement that tests/test_gpu_tap_bnb_epilogue.py and tests/test_gpu_head_final_kernels.py hold the
fused BatchNorm-backward-sum kernels to) is itself checked here, on the CPU:

* against torch autograd in fp64 on conv -> batch_norm(training) -> relu -> 1x1 conv (a 2 x 3 x 5 x 7 toy): ``dbeta = sum g``,
  ``dgamma = sum g*xhat``, the gradient w.r.t. the BatchNorm input ``dy = coef0*(g - coef1 - xhat*coef2)`` with rv_bn_bwd_finalize's
  coefficients, the final conv's weight gradient, and -- the data-grad form -- the same two sums from the gradient w.r.t. the ReLU output;
* the strict ``>`` of the gate at ``t == 0`` exactly;
* that the integer ranges the exact GPU tests use keep every sum of absolute terms below 2^23 at their LARGEST shapes
  (``exactness_margin``; figures printed with ``pytest -s``).  On one x86-64 host: data-grad 3 x 48 x 1024 pixels, 32 -> 128 channels,
  worst sum |g*xhat| 4.6e6; head P = 40000, C = 512, n_out = 26, worst 1.4e6 (sum |g*xhat|; sum |g*y| + |mean| sum |g| 1.1e6).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

import fused_bnb_ref as R


def _toy(relu: bool):
    gen = torch.Generator().manual_seed(3)
    N, cin, H, W, C, n_out = 2, 3, 5, 7, 4, 3
    x = torch.randn(N, cin, H, W, generator=gen, dtype=torch.float64)
    w1 = torch.randn(C, cin, 3, 3, generator=gen, dtype=torch.float64)
    w2 = torch.randn(n_out, C, 1, 1, generator=gen, dtype=torch.float64, requires_grad=True)
    gamma = (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).requires_grad_()
    beta = (0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).requires_grad_()
    dOut = torch.randn(N, n_out, H, W, generator=gen, dtype=torch.float64)
    y = F.conv2d(x, w1, padding=1).requires_grad_()
    eps = 1e-5
    z = F.batch_norm(y, None, None, gamma, beta, training=True, eps=eps)
    a = (F.relu(z) if relu else z)
    a.retain_grad()
    out = F.conv2d(a, w2)
    (out * dOut).sum().backward()
    mean = y.detach().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(y.detach().var((0, 2, 3), unbiased=False) + eps)
    scale = gamma.detach() * invstd
    shift = beta.detach() - mean * scale
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return dict(y=nhwc(y), dY=nhwc(dOut), W=w2.detach().reshape(n_out, C), scale=scale, shift=shift, mean=mean, invstd=invstd, gamma=gamma.detach(),
                dgamma=gamma.grad, dbeta=beta.grad, dy=nhwc(y.grad), dA=nhwc(a.grad), dW=w2.grad.reshape(n_out, C), count=N * H * W)


def _close(a, b, what):
    assert torch.allclose(a, b, rtol=1e-11, atol=1e-12), (what, float((a - b).abs().max()))


def test_reference_against_autograd_fp64():
    for relu in (True, False):
        t = _toy(relu)
        h = R.head_final_ref(t["y"], t["dY"], t["W"], t["scale"], t["shift"], t["mean"], t["invstd"], relu, operand=None)
        _close(h.sum_g, t["dbeta"], "dbeta")
        _close(h.sum_gx, t["dgamma"], "dgamma")
        _close(h.dW, t["dW"], "dW")
        coef = torch.stack([t["gamma"] * t["invstd"], h.sum_g / t["count"], h.sum_gx / t["count"]])  # rv_bn_bwd_finalize (include/rv3d.h)
        h = R.head_final_ref(t["y"], t["dY"], t["W"], t["scale"], t["shift"], t["mean"], t["invstd"], relu, coef=coef, operand=None)
        _close(h.dy, t["dy"], "dy")
        # the data-grad form takes the stored gradient w.r.t. the (activated) BatchNorm output
        _close(h.dA, t["dA"], "dA")
        s0, s1 = R.data_grad_bnb_ref(t["dA"], t["y"], t["scale"], t["shift"], t["mean"], t["invstd"], relu)
        _close(s0, t["dbeta"], "dbeta (data-grad)")
        _close(s1, t["dgamma"], "dgamma (data-grad)")


def test_gate_is_strict_at_zero_and_act_is_rounded_to_the_operand_type():
    y = torch.tensor([[-2.0, 0.0, 2.0, 1.0]])
    scale, shift = torch.tensor([1.0, 1.0, 0.5, 2.0]), torch.tensor([2.0, 0.0, -1.0, -1.0])  # t = 0, 0, 0, 1
    one, zero = torch.ones(4), torch.zeros(4)
    s0, s1 = R.data_grad_bnb_ref(torch.full((1, 4), 3.0), y, scale, shift, zero, one, True)
    assert s0.tolist() == [0.0, 0.0, 0.0, 3.0] and s1.tolist() == [0.0, 0.0, 0.0, 3.0]
    s0, _ = R.data_grad_bnb_ref(torch.full((1, 4), 3.0), y, scale, shift, zero, one, False)
    assert s0.tolist() == [3.0] * 4
    h = R.head_final_ref(torch.full((1, 2), 1.0), torch.ones(1, 1), torch.ones(1, 2), torch.tensor([1.0 + 2 ** -9, 1.0 + 2 ** -12]), torch.zeros(2),
                         torch.zeros(2), torch.ones(2), 1)
    assert h.act.tolist() == [[1.0, 1.0]]  # (bf16: 8 bits of significand)
    h = R.head_final_ref(torch.full((1, 2), 1.0), torch.ones(1, 1), torch.ones(1, 2), torch.tensor([1.0 + 2 ** -9, 1.0 + 2 ** -12]), torch.zeros(2),
                         torch.zeros(2), torch.ones(2), 1, operand=torch.float16)
    assert h.act.tolist() == [[1.0 + 2 ** -9, 1.0]]


def test_integer_ranges_of_the_exact_tests_stay_below_the_margin():
    """The largest shapes of the exact GPU tests, the operand recipes they use."""
    gen = torch.Generator().manual_seed(1)
    # rv_tap_data_grad_bnb: weights -1..1, dout -3..3, y -2..2 (fused_bnb_ref.data_grad_bn); 32 -> 128 channels at 3 x 48 x 1024
    N, H, W, cs, cd = 3, 48, 1024, 32, 128
    w = torch.randint(-1, 2, (cs, cd, 3, 3), generator=gen).float()
    dout = torch.randint(-3, 4, (N, cs, H, W), generator=gen).float()
    dx = F.conv_transpose2d(dout, w, padding=1)
    assert float(dx.abs().max()) < 2 ** 24
    dx = dx.bfloat16().double().permute(0, 2, 3, 1)
    y = torch.randint(-2, 3, (N, H, W, cd), generator=gen).double()
    scale, shift, mean, invstd = R.data_grad_bn(cd, gen)
    m = R.exactness_margin(dx * R.gate(y, scale, shift, False), (y - mean) * invstd)
    print("data-grad margins", {k: float(v.max()) for k, v in m.items()})
    R.assert_exact(m)
    # head-final: y -3..3, dY and W -2..2 at P = 40000, C = 512, n_out = 26, invstd any signed power of two in [1/4, 2]
    P, C, n_out = 40000, 512, 26
    y = torch.randint(-3, 4, (P, C), generator=gen).double()
    dY = torch.randint(-2, 3, (P, n_out), generator=gen).double()
    Wt = torch.randint(-2, 3, (n_out, C), generator=gen).double()
    scale, shift, mean, invstd, _ = R.head_bn(C, gen)
    for relu in (0, 1):
        h = R.head_final_ref(y, dY, Wt, scale, shift, mean, invstd, relu)
        m = R.exactness_margin(h.g, h.xhat, dY, h.act, y, mean)
        print("head-final margins, relu", relu, {k: float(v.max()) for k, v in m.items()})
        R.assert_exact(m)
