"""Records what the conv host path launches: every ``_lib.call`` of a set of small conv programs, as plain data.

    python tests/tools/record_conv_route_trace.py [out.json]      (default: tests/golden/conv_route_trace.json; needs an MI355X)

A row is one library call: the entry point, whether the current stream is the side stream, and its arguments by their parameter
names in include/rv3d.h -- scalars by value, ``rvTapGeom`` / ``rvTapShape`` / ``rvBnbEpilogue`` field by field, pointers only as
"null or not".  Event records and stream waits are rows too (``event.record`` / ``stream.wait_event``): they are what orders the
weight gradient against the backward-data launch.  Per case the calls of ``_lib.tap_launch_info`` (planning queries) are counted.

The file under tests/golden/ was recorded BEFORE the launch decisions moved into ``conv_route``; tests/test_gpu_conv_route_trace.py
demands the same rows of the current tree.  It is re-recorded only by a change that means to alter a launch.
"""

from __future__ import annotations

import contextlib
import ctypes
import json
import os
import sys
from typing import Callable, Dict, List

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_route_trace.json")


def _plain(ctype, v):
    """One argument as JSON data."""
    if isinstance(v, ctypes.Structure):
        return {n: ({"null": not getattr(v, n)} if t is ctypes.c_void_p else getattr(v, n)) for n, t in v._fields_}
    if ctype in (ctypes.c_int32, ctypes.c_int64):
        return int(v)
    if ctype in (ctypes.c_float, ctypes.c_double):
        return float(v)
    return {"null": v is None or (isinstance(v, ctypes.c_void_p) and not v.value)}


@contextlib.contextmanager
def recording(rows: List[dict], queries: List[int]):
    """Inside: every ``_lib.call``, event record and stream wait is appended to ``rows``; ``queries[0]`` counts ``_lib.tap_launch_info``."""
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    protos = {**L.included_prototypes(), **L.companion_prototypes(), **L.prototypes()}
    on_side = lambda: torch.cuda.current_stream() in E._SIDE_STREAMS.values()
    real = L.call, L.tap_launch_info, torch.cuda.Event.record, torch.cuda.Stream.wait_event

    def call(name, *args):
        rows.append({"fn": name, "side": on_side(), "args": {p: _plain(c, a) for (c, p), a in zip(protos[name][1], args)}})
        return real[0](name, *args)

    def launch_info(*a):
        queries[0] += 1
        return real[1](*a)

    def record(ev, *a):
        rows.append({"fn": "event.record", "side": on_side(), "args": {}})
        return real[2](ev, *a)

    def wait_event(stream, ev):
        rows.append({"fn": "stream.wait_event", "side": stream in E._SIDE_STREAMS.values(), "args": {}})
        return real[3](stream, ev)

    L.call, L.tap_launch_info, torch.cuda.Event.record, torch.cuda.Stream.wait_event = call, launch_info, record, wait_event
    try:
        yield
    finally:
        L.call, L.tap_launch_info, torch.cuda.Event.record, torch.cuda.Stream.wait_event = real


@contextlib.contextmanager
def switched(**switches):
    """Module switches of ``engine`` / ``engine_bwd`` set for the block (``HEAD_FINAL_FUSE`` lives in engine_bwd)."""
    from range_view_3d_detection_amd import engine as E
    from range_view_3d_detection_amd import engine_bwd

    where = {k: (E if hasattr(E, k) else engine_bwd) for k in switches}
    old = {k: getattr(where[k], k) for k in switches}
    for k, v in switches.items():
        setattr(where[k], k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(where[k], k, v)


DEV = "cuda:0"


def _conv(cin: int, cout: int, k, stride: int = 1, bias: bool = False):
    k = (k, k) if isinstance(k, int) else k
    return torch.nn.Conv2d(cin, cout, k, stride=(1, stride), padding=((k[0] - 1) // 2, (k[1] - 1) // 2), bias=bias).to(DEV)


def _convT(cin: int, cout: int, k, stride: int, pad):
    return torch.nn.ConvTranspose2d(cin, cout, k, stride=(1, stride), padding=pad, bias=False).to(DEV)


def _train(build: Callable) -> None:
    """Forward + backward of ``build(tape) -> ConvOp`` in training mode, gradient of ones."""
    from range_view_3d_detection_amd import engine as E
    from range_view_3d_detection_amd import engine_bwd

    t = E.Tape(True, torch.device(DEV))
    op = build(t)
    if op.out_f32:
        n, h, w = op.out_t.shape[:3]
        engine_bwd.seed_f32_output_grad(t, op, torch.ones((n, op.layer.c_out, h, w), device=DEV))
    else:
        g = op.out.like()
        g.data.fill_(1.0)
        t.set_grad(op.out, g)
    t.backward()


def _x(c: int, n: int, h: int, w: int):
    from range_view_3d_detection_amd import engine as E

    return E.Act.from_nchw(torch.ones((n, c, h, w), device=DEV))


def chain(c0: int, c1: int, second, n: int, h: int, w: int, first_grad: bool = True, **conv_kw) -> Callable:
    """conv3x3(c0 -> c1) -> BatchNorm -> ReLU -> ``second`` (a module taking c1 channels), statistics on unless ``conv_kw`` says otherwise;
    ``first_grad=False``: the input of the first conv needs no gradient (no backward-data launch at all)."""
    from range_view_3d_detection_amd import engine as E

    first, bn = _conv(c0, c1, 3), torch.nn.BatchNorm2d(c1).to(DEV).train()
    conv_kw.setdefault("stats", True)
    return lambda: _train(lambda t: E.ConvOp(t, E.tap_layer(second), E.conv_bn(t, E.tap_layer(first), _x(c0, n, h, w), bn, need_input_grad=first_grad), **conv_kw))


def single(module, c: int, n: int, h: int, w: int) -> Callable:
    from range_view_3d_detection_amd import engine as E

    return lambda: _train(lambda t: E.ConvOp(t, E.tap_layer(module), _x(c, n, h, w)))


def evaluated(module, c: int, n: int, h: int, w: int, residual: bool = False) -> Callable:
    """Eval mode, forward only: conv + folded BatchNorm + ReLU, or the residual form."""
    from range_view_3d_detection_amd import engine as E

    bn = torch.nn.BatchNorm2d(module.out_channels).to(DEV).eval()

    def run():
        with torch.no_grad():
            t = E.Tape(False, torch.device(DEV))
            if residual:
                assert E.conv_bn_residual(t, E.tap_layer(module), _x(c, n, h, w), bn, _x(module.out_channels, n, h, w), False, True) is not None
            else:
                E.conv_bn(t, E.tap_layer(module), _x(c, n, h, w), bn)

    return run


def cases() -> Dict[str, Callable]:
    """name -> (select flags, switches, builder of the program); a builder makes fresh modules, so no layer state is shared."""
    from range_view_3d_detection_amd import _lib as L

    small = L.SEL_SMALL_GRIDS | L.SEL_SMALL_GRIDS6
    out: Dict[str, tuple] = {}

    def add(name, make, sel=small, **switches):
        out[name] = (sel, switches, make)

    add("dma_3x3_128", lambda: chain(128, 128, _conv(128, 128, 3), 1, 16, 64))
    add("dma_3x3_128_no_bnb", lambda: chain(128, 128, _conv(128, 128, 3), 1, 16, 64), BNB_FUSE=False)
    add("dma_3x3_128_no_write_out", lambda: chain(128, 128, _conv(128, 128, 3), 1, 16, 64), MATERIALIZE_FOR_DMA=False)
    add("dma_3x3_128_h8", lambda: chain(128, 128, _conv(128, 128, 3), 1, 8, 64))
    add("pointwise_256", lambda: chain(256, 256, _conv(256, 256, 1), 1, 16, 64))
    add("pointwise_128", lambda: chain(128, 128, _conv(128, 128, 1), 1, 16, 64))
    strided = {"s2_3x3": (lambda: _conv(128, 128, 3, 2), 128, 256), "s2_1x1": (lambda: _conv(128, 256, 1, 2), 128, 256),
               "convT_3x8_s4": (lambda: _convT(128, 256, (3, 8), 4, (1, 2)), 128, 64), "convT_3x4_s2": (lambda: _convT(128, 128, (3, 4), 2, (1, 1)), 128, 128)}
    for name, (make, c, w) in strided.items():
        add(name + "_fold", lambda make=make, c=c, w=w: single(make(), c, 2, 8, w))
        add(name + "_no_fold", lambda make=make, c=c, w=w: single(make(), c, 2, 8, w), FOLD_STRIDED=False)
    add("s2_3x3_after_bn", lambda: chain(128, 128, _conv(128, 128, 3, 2), 2, 8, 256))  # (write-out for the folded view)
    add("basic_3x3_64", lambda: chain(64, 64, _conv(64, 64, 3), 1, 16, 64))
    add("basic_3x3_64_no_input_grad", lambda: chain(64, 64, _conv(64, 64, 3), 1, 16, 64, first_grad=False))
    add("tower_end", lambda: chain(256, 256, _conv(256, 26, 1, bias=True), 1, 16, 64, stats=False, out_f32=True))
    add("tower_end_no_fuse", lambda: chain(256, 256, _conv(256, 26, 1, bias=True), 1, 16, 64, stats=False, out_f32=True), HEAD_FINAL_FUSE=False)
    add("full_round_gen6", lambda: single(_conv(128, 128, 3), 128, 1, 64, 2048), sel=0)
    add("eval_fold_relu", lambda: evaluated(_conv(128, 128, 3), 128, 1, 16, 64))
    add("eval_residual", lambda: evaluated(_conv(128, 128, 3), 128, 1, 16, 64, residual=True))
    add("eval_s2_3x3", lambda: evaluated(_conv(128, 128, 3, 2), 128, 2, 8, 256))
    return out


def record() -> Dict[str, dict]:
    from range_view_3d_detection_amd import _lib as L

    trace = {}
    for name, (sel, switches, make) in cases().items():
        rows, queries = [], [0]
        with L.select(sel), switched(**switches):
            run = make()
            with recording(rows, queries):
                run()
        torch.cuda.synchronize()
        trace[name] = {"tap_launch_info": queries[0], "rows": rows}
    return trace


def dump(trace: Dict[str, dict], path: str) -> None:
    """One row per line: a change shows as a line in a diff."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (name, case) in enumerate(trace.items()):
            f.write(f' {json.dumps(name)}: {{"tap_launch_info": {case["tap_launch_info"]}, "rows": [\n')
            f.write(",\n".join("  " + json.dumps(r, sort_keys=True) for r in case["rows"]))
            f.write("\n ]}" + (",\n" if i + 1 < len(trace) else "\n"))
        f.write("}\n")


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    recorded = record()
    dump(recorded, out_path)
    print(f"{sum(len(c['rows']) for c in recorded.values())} rows of {len(recorded)} cases -> {out_path}")
