"""The conv host path issues the launches it issued before its decisions moved into ``conv_route``: every library call of a set of
small conv programs (tests/tools/record_conv_route_trace.py: entry point, scalar arguments, ``rvTapGeom`` / ``rvTapShape`` /
``rvBnbEpilogue`` fields, null-ness of pointers, side stream or not, event records and waits) against tests/golden/conv_route_trace.json,
recorded on an MI355X with the engine as it was before.  The planning queries (``_lib.tap_launch_info``) per case may only go down."""

from __future__ import annotations

import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def traces():
    import record_conv_route_trace as rec

    with open(rec.GOLDEN) as f:
        golden = json.load(f)
    return golden, json.loads(json.dumps(rec.record()))  # (through JSON: the same types on both sides)


def test_same_launches_as_recorded(traces):
    golden, now = traces
    assert list(now) == list(golden)
    for name, want in golden.items():
        got = now[name]
        assert len(got["rows"]) == len(want["rows"]), (name, [r["fn"] for r in got["rows"]], [r["fn"] for r in want["rows"]])
        for i, (g, w) in enumerate(zip(got["rows"], want["rows"])):
            assert g == w, (name, i, g, w)
        assert got["tap_launch_info"] <= want["tap_launch_info"], (name, got["tap_launch_info"], want["tap_launch_info"])


def test_recorded_cases_cover_every_route_form(traces):
    """A condition on the INPUTS: the golden trace itself holds each write-out reason, each backward-data form, both weight-gradient
    forms, the fused epilogue, the residual form, a side-stream launch and both sides of the early-release rule."""
    golden, _ = traces
    rows = {name: case["rows"] for name, case in golden.items()}
    fns = lambda name: [r["fn"] for r in rows[name]]
    taps = lambda name, fn: [r["args"] for r in rows[name] if r["fn"] == fn]

    def written_out_then(name, kh, kw, cv, stride=1):  # rv_ew_combine, then the gather on this geometry
        f = fns(name)
        g = taps(name, "rv_tap_gather")[-1]["g"]
        return "rv_ew_combine" in f and f.index("rv_ew_combine") < len(f) - f[::-1].index("rv_tap_gather") - 1 and \
            (g["kh"], g["kw"], g["cv"], g["stride_w"]) == (kh, kw, cv, stride)

    assert written_out_then("dma_3x3_128", 3, 3, 128)                        # write-out: dma
    assert written_out_then("pointwise_256", 1, 1, 256)                      # write-out: pointwise
    assert written_out_then("s2_3x3_after_bn", 3, 2, 256)                    # write-out: folded (the stride-1 view of the 3x3 s2 layer)
    assert "rv_ew_combine" not in fns("pointwise_128") + fns("dma_3x3_128_no_write_out") + fns("basic_3x3_64")
    # backward-data: plain, folded (a stride-1 gather over 4 * 256 channels), even columns (destination pitch doubled), none
    assert taps("s2_3x3_fold", "rv_tap_scatter")[0]["g"]["stride_w"] == 2
    g, s = (taps("convT_3x8_s4_fold", "rv_tap_gather")[0][k] for k in "gs")
    assert (g["kw"], g["stride_w"], g["cv"], s["ld_src"]) == (3, 1, 1024, 1024)
    g, s = (taps("s2_1x1_fold", "rv_tap_scatter")[0][k] for k in "gs")
    assert (g["stride_w"], s["Wv"], s["ld_dst"]) == (1, 128, 256) and taps("s2_1x1_no_fold", "rv_tap_scatter")[0]["s"]["ld_dst"] == 128
    assert fns("basic_3x3_64_no_input_grad").count("rv_tap_scatter") == 1 and fns("basic_3x3_64").count("rv_tap_scatter") == 2
    # weight gradient: folded + unfold, and on the layer's own geometry
    assert "rv_unfold_weight_grad" in fns("s2_3x3_fold") and taps("s2_3x3_fold", "rv_tap_wgrad")[0]["ld_v"] == 256
    assert "rv_unfold_weight_grad" not in fns("s2_3x3_no_fold") and taps("s2_3x3_no_fold", "rv_tap_wgrad")[0]["ld_v"] == 128
    assert "rv_tap_data_grad_bnb" in fns("dma_3x3_128") and "rv_tap_data_grad_bnb" not in fns("dma_3x3_128_no_bnb")
    assert "rv_tap_residual" in fns("eval_residual") and "rv_head_final_bwd_sums" in fns("tower_end")
    wgrads = [r for name in rows for r in rows[name] if r["fn"] == "rv_tap_wgrad"]
    assert len(wgrads) >= 20 and all(r["side"] for r in wgrads)  # side-stream launches (the default overlap: every weight gradient)
    # early release: the event the weight gradient waits for is recorded BEFORE the backward-data launch / after it
    early, late = fns("dma_3x3_128"), fns("full_round_gen6")
    assert early.index("event.record") + 1 == early.index("rv_tap_data_grad_bnb")
    assert late.index("rv_tap_scatter") + 1 == late.index("event.record")
