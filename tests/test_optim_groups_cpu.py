"""Parameter groups of the training recipe without a GPU: ``configure_optimizers``' ``weight_decay`` / ``no_weight_decay_1d`` keywords
(``nn/meta/arch.py``) on ``torch.optim.AdamW``, and the declaration, typing and export of ``rv_adamw_step_groups`` (``include/rv3d_optim.h``)."""

from __future__ import annotations

import ctypes
import math
import os

import pytest
import torch

from range_view_3d_detection_amd.nn.meta.arch import configure_optimizers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, bias=False), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1, bias=True))


@pytest.mark.parametrize("named", [True, False])
def test_no_weight_decay_1d_gives_two_groups(named):
    net = _net()
    params = net.named_parameters() if named else net.parameters()
    opt, sched = configure_optimizers(params, num_devices=2, batch_size=4, total_steps=10, weight_decay=0.05, no_weight_decay_1d=True, fused=False)
    assert isinstance(opt, torch.optim.AdamW) and len(opt.param_groups) == 2
    decay, no_decay = opt.param_groups
    assert [id(p) for p in decay["params"]] == [id(net[0].weight), id(net[2].weight)] and decay["weight_decay"] == 0.05
    assert [id(p) for p in no_decay["params"]] == [id(net[1].weight), id(net[1].bias), id(net[2].bias)] and no_decay["weight_decay"] == 0.0
    assert all(p.ndim >= 2 for p in decay["params"]) and all(p.ndim <= 1 for p in no_decay["params"])
    # OneCycleLR carries the scaled max_lr in both groups, and starts both at max_lr / 25
    want = 0.00075 * math.sqrt(2 * 4)
    assert isinstance(sched, torch.optim.lr_scheduler.OneCycleLR)
    for g in opt.param_groups:
        assert g["max_lr"] == want and g["lr"] == pytest.approx(want / 25.0, rel=1e-12)


def test_defaults_give_todays_single_group():
    net = _net()
    opt, sched = configure_optimizers(net.parameters(), num_devices=1, batch_size=4, total_steps=10, fused=False)
    ref = torch.optim.AdamW(list(net.parameters()), lr=1e-3)
    ref_sched = torch.optim.lr_scheduler.OneCycleLR(ref, max_lr=0.00075 * 2.0, total_steps=10)
    assert len(opt.param_groups) == 1 and [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in net.parameters()]
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    assert opt.param_groups[0]["weight_decay"] == 1e-2 and sched.total_steps == ref_sched.total_steps
    # weight_decay alone is passed through
    opt, _ = configure_optimizers(net.parameters(), num_devices=1, batch_size=4, total_steps=10, fused=False, weight_decay=0.2, debug=True)
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["weight_decay"] == 0.2


def test_group_dicts_pass_through_and_the_split_refuses_them():
    net = _net()
    groups = [{"params": [net[0].weight], "lr": 1e-4}, {"params": [net[2].weight, net[2].bias], "weight_decay": 0.0}]
    opt, _ = configure_optimizers(groups, num_devices=1, batch_size=4, total_steps=10, fused=False)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 2] and opt.param_groups[1]["weight_decay"] == 0.0
    assert opt.param_groups[0]["max_lr"] == opt.param_groups[1]["max_lr"] == 0.00075 * 2.0
    with pytest.raises(TypeError, match="no_weight_decay_1d"):
        configure_optimizers(groups, num_devices=1, batch_size=4, total_steps=10, fused=False, no_weight_decay_1d=True)


def test_grouped_step_is_declared_typed_and_exported():
    """``rv_adamw_step_groups`` / ``rv_adam_max_rows`` are declared in ``include/rv3d_optim.h`` (a companion of ``rv3d.h`` with a table
    of its own, as ``rv3d_render.h``), typed from it on both builds, and ``rvAdamRow`` is mirrored field by field."""
    from range_view_3d_detection_amd import _lib as L

    protos = L.optim_prototypes()
    assert sorted(protos) == ["rv_adam_max_rows", "rv_adamw_step_groups"]
    assert not set(protos) & (set(L.prototypes()) | set(L.included_prototypes()) | set(L.companion_prototypes()))
    restype, params = protos["rv_adamw_step_groups"]
    assert restype is ctypes.c_int32 and [n for _, n in params] == ["tensors", "tensor_row", "vmax", "chunks", "n_chunks", "partial", "rows", "n_rows",
                                                                     "max_norm", "total_norm", "stream"]
    assert dict((n, t) for t, n in params)["rows"] is ctypes.POINTER(L.AdamRow) and dict((n, t) for t, n in params)["max_norm"] is ctypes.c_double
    header = open(os.path.join(ROOT, "include", "rv3d_optim.h")).read()
    assert '#include "rv3d.h"' in header and "#define RV_ADAM_AMSGRAD 1" in header and "#define RV_ADAM_MAXIMIZE 2" in header
    assert (L.ADAM_AMSGRAD, L.ADAM_MAXIMIZE) == (1, 2)
    assert "double lr, beta1, beta2, eps, weight_decay;" in header and "int64_t step;" in header and "int32_t flags;" in header
    assert [(n, t) for n, t in L.AdamRow._fields_] == [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + \
        [("step", ctypes.c_int64), ("flags", ctypes.c_int32)]
    for tag in ("bf16", "f16"):
        handle = L.load(tag)  # (load() raises if a declared symbol is not exported)
        cap = handle.rv_adam_max_rows()
        assert 1 <= cap and cap * 32 + 64 <= 3072  # rows of 7 floats + flags by value, well under the 4 KB of kernel arguments
        assert handle.rv_adamw_step_groups.argtypes is not None
    # refused on the host, before any launch: no rows, too many rows, an amsgrad row without the max_exp_avg_sq table
    x = ctypes.c_void_p(16)
    rows = (L.AdamRow * 1)(L.AdamRow(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0))
    for n_rows, flags, word in ((0, 0, "rv_adam_max_rows"), (cap + 1, 0, "rv_adam_max_rows"), (1, L.ADAM_AMSGRAD, "vmax")):
        rows[0].flags = flags
        with pytest.raises(L.RvError, match=word):
            L.call("rv_adamw_step_groups", x, x, None, x, 1, x, rows, n_rows, 0.0, None, None)


def test_constructor_takes_torchs_keywords():
    from range_view_3d_detection_amd.optim import AdamW

    p = [torch.nn.Parameter(torch.zeros(3))]
    opt = AdamW(p, lr=1e-3, amsgrad=True, maximize=True, foreach=False, fused=True, max_grad_norm=35.0)
    ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, amsgrad=True, maximize=True)
    assert set(opt.param_groups[0]) == set(ref.param_groups[0])
    assert opt.param_groups[0]["amsgrad"] is True and opt.param_groups[0]["maximize"] is True and opt.max_grad_norm == 35.0
    assert opt.param_groups[0]["fused"] is None and opt.param_groups[0]["foreach"] is None  # accepted and ignored
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "amsgrad": False})
    assert opt.param_groups[1]["amsgrad"] is False and opt.param_groups[1]["maximize"] is True
    for kw in ("capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=kw):
            AdamW(p, **{kw: True})
