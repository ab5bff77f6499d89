"""Weight averaging without a GPU: the host function that picks the weight of an update (``optim.average_weight``) against what
``torch.optim.swa_utils``' multi-tensor functions apply, the declaration and typing of ``rv_adamw_step_groups_avg`` /
``rv_average_tensors`` (``include/rv3d_optim.h``), their refusals (made on the host, before any launch), and the routes of
``optim.AveragedModel`` that are torch's own (a CPU model, a custom ``avg_fn``)."""

from __future__ import annotations

import copy
import ctypes
import os

import pytest
import torch
from torch.optim.swa_utils import get_ema_multi_avg_fn, get_swa_multi_avg_fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("decay", [None, 0.9, 0.999])
def test_weight_of_an_update_is_torchs(decay):
    """Six updates of three CPU tensors: ``lerp(averaged, current, average_weight(n, decay))`` (a copy at n = 0, as ``AveragedModel`` does
    it) equals, bit for bit, what ``get_swa_multi_avg_fn()`` / ``get_ema_multi_avg_fn(decay)`` leave behind."""
    from range_view_3d_detection_amd.optim import average_weight

    assert average_weight(0, decay) == 1.0
    for n in range(1, 7):
        assert average_weight(n, decay) == (1.0 / (n + 1) if decay is None else 1.0 - decay)
    with pytest.raises(ValueError):
        average_weight(-1, decay)
    gen = torch.Generator().manual_seed(0)
    fn = get_swa_multi_avg_fn() if decay is None else get_ema_multi_avg_fn(decay)
    ours = [torch.zeros(s) for s in ((5,), (3, 7), (1,))]
    theirs = [t.clone() for t in ours]
    for n in range(6):
        current = [torch.randn(t.shape, generator=gen) for t in ours]
        w = average_weight(n, decay)
        for a, p in zip(ours, current):
            a.copy_(p) if n == 0 else a.lerp_(p, w)
        if n == 0:
            for a, p in zip(theirs, current):
                a.copy_(p)
        else:
            fn(theirs, current, n)
        assert all(torch.equal(a, b) for a, b in zip(ours, theirs)), n
    assert not torch.equal(ours[0], current[0])


def test_entries_are_declared_typed_and_exported():
    from range_view_3d_detection_amd import _lib as L

    protos = L.average_prototypes()
    assert sorted(protos) == ["rv_adamw_step_groups_avg", "rv_average_tensors"]
    header = open(os.path.join(ROOT, "include", "rv3d_optim.h")).read()
    assert "int rv_adamw_step_groups_avg(" in header and "int rv_average_tensors(" in header
    restype, params = protos["rv_adamw_step_groups_avg"]
    names = [n for _, n in params]
    assert restype is ctypes.c_int32 and names == ["tensors", "tensor_row", "vmax", "avg", "avg_weight", "chunks", "n_chunks", "partial", "rows",
                                                    "n_rows", "max_norm", "total_norm", "stream"]
    # rv_adamw_step_groups plus the two arguments, nothing else moved
    assert [n for n in names if n not in ("avg", "avg_weight")] == [n for _, n in L.optim_prototypes()["rv_adamw_step_groups"][1]]
    types = dict((n, t) for t, n in params)
    assert types["avg"] is ctypes.c_void_p and types["avg_weight"] is ctypes.c_double and types["rows"] is ctypes.POINTER(L.AdamRow)
    restype, params = protos["rv_average_tensors"]
    assert restype is ctypes.c_int32 and [n for _, n in params] == ["table", "chunks", "n_chunks", "avg_weight", "stream"]
    assert [t for t, _ in params] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p]
    for tag in ("bf16", "f16"):
        handle = L.load(tag)  # (load() raises if a declared symbol is not exported)
        assert handle.rv_adamw_step_groups_avg.argtypes is not None and handle.rv_average_tensors.argtypes is not None


def test_refusals_on_the_host():
    """Non-zero and a message before anything is launched: null arguments, a weight outside [0, 1] (NaN too), bad rows."""
    from range_view_3d_detection_amd import _lib as L

    x = ctypes.c_void_p(16)
    for args, word in (((None, x, 1, 0.5, None), "null"), ((x, None, 1, 0.5, None), "null"), ((x, x, 0, 0.5, None), "n_chunks"),
                       ((x, x, 1, -0.01, None), "avg_weight"), ((x, x, 1, 1.5, None), "avg_weight"), ((x, x, 1, float("nan"), None), "avg_weight")):
        with pytest.raises(L.RvError, match=word):
            L.call("rv_average_tensors", *args)
    rows = (L.AdamRow * 1)(L.AdamRow(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, 0))
    cap = L.load().rv_adam_max_rows()
    for avg, w, n_rows, flags, word in ((None, 0.5, 1, 0, "null"), (x, 1.0001, 1, 0, "avg_weight"), (x, -1.0, 1, 0, "avg_weight"),
                                        (x, 0.5, 0, 0, "rv_adam_max_rows"), (x, 0.5, cap + 1, 0, "rv_adam_max_rows"), (x, 0.5, 1, L.ADAM_AMSGRAD, "vmax")):
        rows[0].flags = flags
        with pytest.raises(L.RvError, match=word):
            L.call("rv_adamw_step_groups_avg", x, x, None, avg, w, x, 1, x, rows, n_rows, 0.0, None, None)


def _net():
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 1), torch.nn.BatchNorm2d(3))


@pytest.mark.parametrize("use_buffers", [False, True])
@pytest.mark.parametrize("decay", [None, 0.9])
def test_cpu_model_takes_torchs_path(decay, use_buffers):
    """A CPU model: torch's own ``update_parameters`` (equal results and state-dict keys), ``requires_grad`` off on the averaged copy, and
    ``fuse`` refuses."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.optim import AdamW, AveragedModel

    torch.manual_seed(0)
    net = _net()
    ours = AveragedModel(net, use_buffers=use_buffers, decay=decay)
    theirs = torch.optim.swa_utils.AveragedModel(net, multi_avg_fn=None if decay is None else get_ema_multi_avg_fn(decay), use_buffers=use_buffers)
    assert isinstance(ours, torch.optim.swa_utils.AveragedModel) and not ours._native
    assert all(not p.requires_grad for p in ours.module.parameters()) and all(p.requires_grad for p in net.parameters())
    for _ in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn(p.shape))
        net(torch.randn(2, 2, 3, 3))
        ours.update_parameters(net)
        theirs.update_parameters(net)
    a, b = ours.state_dict(), theirs.state_dict()
    assert list(a) == list(b) and list(a)[0] == "n_averaged" and all(k.startswith("module.") for k in list(a)[1:])
    assert all(torch.equal(a[k], b[k]) for k in a) and int(a["n_averaged"]) == 3
    with pytest.raises(L.RvError, match="fuse"):
        ours.fuse(AdamW(list(net.parameters())), net)
    theirs.load_state_dict(copy.deepcopy(a))
    ours.load_state_dict(copy.deepcopy(b))


def test_custom_functions_and_bad_decay():
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.optim import AdamW, AveragedModel

    net = _net()
    custom = AveragedModel(net, avg_fn=lambda a, p, n: 0.5 * a + 0.5 * p)
    assert not custom._native
    with pytest.raises(L.RvError, match="fuse"):
        custom.fuse(AdamW(list(net.parameters())), net)
    with pytest.raises(ValueError):
        AveragedModel(net, decay=1.5)
    with pytest.raises(ValueError):
        AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(0.9), decay=0.9)
