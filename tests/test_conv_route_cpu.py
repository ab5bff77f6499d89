"""The launch decisions of the conv host path (``conv_route``) on plain values, without a GPU: which forward form, whether a folded
BatchNorm operand is written out first and why, which backward-data form, the early release of the weight gradient, which weight-gradient
form.  The expected planner answers are those of the library for 256 CUs (what it plans for without a device)."""

from __future__ import annotations

import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256


@pytest.fixture(scope="module")
def mods():
    from range_view_3d_detection_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "range_view_3d_detection_amd", "csrc"), "-j8"], check=True)
    from range_view_3d_detection_amd import conv_route, engine

    return _lib, engine, conv_route


@pytest.fixture
def switch(mods, monkeypatch):
    return lambda name, value: monkeypatch.setattr(mods[1], name, value)


def conv(E, cin, cout, k, stride=1, bias=False):
    k = (k, k) if isinstance(k, int) else k
    return E.tap_layer(torch.nn.Conv2d(cin, cout, k, stride=(1, stride), padding=((k[0] - 1) // 2, (k[1] - 1) // 2), bias=bias))


def fields(s):
    return tuple(getattr(s, n) for n, _ in s._fields_)


def forward(mods, layer, n, h, w, lazy=False, out_flags=0, ld=None, ld_dst=None):
    L, E, R = mods
    cp = E.pad32(layer.c_in)
    return R.forward_route(layer, n, h, w, cp if ld is None else ld, cp, (L.IN_AFFINE | L.IN_RELU) if lazy else 0,
                           E.pad32(layer.c_out) if ld_dst is None else ld_dst, out_flags)


def dgrad(mods, layer, fwd, accumulate=False, dout_ld=None, bn_operand=False):
    """Backward-data behind ``fwd`` with dense tensors unless ``dout_ld`` says otherwise."""
    L, E, R = mods
    ci, co = E.pad32(layer.c_in), E.pad32(layer.c_out)
    w_in, w_out = (fwd.own.Wu, fwd.own.Wv) if layer.transposed else (fwd.own.Wv, fwd.own.Wu)
    return R.dgrad_route(layer, fwd.own, w_out, co if dout_ld is None else dout_ld, co, w_in, ci, ci, accumulate, bn_operand, lambda: CUS)


def wgrad(mods, layer, fwd):
    """Weight gradient behind ``fwd``: the layer input is what the forward read (plain when it was written out or was plain)."""
    L, E, R = mods
    in_flags = fwd.own.flags & (L.IN_AFFINE | L.IN_RELU)
    c = E.pad32(layer.c_out if layer.transposed else layer.c_in)
    return R.wgrad_route(layer, fwd.own, in_flags, fwd.own.Wv, c, c)


# ---- forward: write-out for the LDS-DMA kernels ----------------------------------------------------------------------------------
def test_3x3_folded_operand_is_written_out_for_dma(mods, switch):
    L, E, R = mods
    layer = conv(E, 256, 256, 3)
    r = forward(mods, layer, 4, 64, 2048, lazy=True, out_flags=L.OUT_STATS)
    assert r.write_out == "dma" and r.shape.flags == L.OUT_STATS and r.own.flags == L.OUT_STATS
    assert r.info == (6, 128, 1024, 2) and r.image == "gather" and fields(r.geom) == (3, 3, 1, 1, 1, 256, 256)
    assert r.rows == 4 * 128
    switch("MATERIALIZE_FOR_DMA", False)
    r = forward(mods, layer, 4, 64, 2048, lazy=True, out_flags=L.OUT_STATS)
    assert r.write_out is None and r.shape.flags == L.IN_AFFINE | L.IN_RELU | L.OUT_STATS and r.info[0] == 2


def test_fp32_output_never_writes_the_operand_out(mods):
    L, E, R = mods
    for layer in (conv(E, 256, 256, 3), conv(E, 256, 256, 1), conv(E, 128, 128, 3, 2)):
        r = forward(mods, layer, 4, 64, 2048, lazy=True, out_flags=L.OUT_F32)
        assert r.write_out is None and r.shape.flags == L.IN_AFFINE | L.IN_RELU | L.OUT_F32


# ---- forward: write-out for the pointwise streaming GEMM -------------------------------------------------------------------------
def test_pointwise_write_out(mods, switch):
    L, E, R = mods
    for out_flags in (0, L.OUT_STATS):
        r = forward(mods, conv(E, 256, 256, 1), 4, 64, 2048, lazy=True, out_flags=out_flags)
        assert r.write_out == "pointwise" and r.info[0] == 7 and r.shape.flags == out_flags
    # 128 is not in MATERIALIZE_POINTWISE_C, although the plain launch would be generation 7
    l128 = conv(E, 128, 128, 1)
    r = forward(mods, l128, 4, 64, 2048, lazy=True, out_flags=L.OUT_STATS)
    assert r.write_out is None and r.shape.flags & L.IN_AFFINE
    assert forward(mods, l128, 4, 64, 2048, out_flags=L.OUT_STATS).info[0] == 7
    # a bias, or an eval fold (both travel as OUT_BIAS): not written out
    assert forward(mods, conv(E, 256, 256, 1, bias=True), 4, 64, 2048, lazy=True, out_flags=L.OUT_BIAS).write_out is None
    assert forward(mods, conv(E, 256, 256, 1), 4, 64, 2048, lazy=True, out_flags=L.OUT_BIAS | L.OUT_RELU).write_out is None
    switch("MATERIALIZE_FOR_POINTWISE", False)
    assert forward(mods, conv(E, 256, 256, 1), 4, 64, 2048, lazy=True).write_out is None


# ---- strided layers on the folded view ------------------------------------------------------------------------------------------
def test_stride2_conv_on_the_folded_view(mods, switch):
    L, E, R = mods
    layer = conv(E, 128, 128, 3, 2)
    r = forward(mods, layer, 4, 64, 2048)
    assert r.write_out is None and r.image == "folded" and fields(r.geom) == (3, 2, 1, 1, 1, 128, 256)
    assert (r.shape.Wu, r.shape.Wv, r.shape.ld_src) == (1024, 1024, 256) and r.info == (6, 128, 512, 1)
    assert (r.own.Wu, r.own.Wv, r.own.ld_src) == (1024, 2048, 128)  # ConvOp.shape stays in the layer's own geometry
    w = wgrad(mods, layer, r)
    assert w.unfold and w.v_pitch == 2 and fields(w.geom) == (3, 2, 1, 1, 1, 128, 256) and (w.shape.Wu, w.shape.Wv) == (1024, 1024)
    assert w.generation == 3
    # fed a folded BatchNorm operand: written out for the folded view, then the same launch
    lz = forward(mods, layer, 4, 64, 2048, lazy=True)
    assert lz.write_out == "folded" and lz.image == "folded" and fields(lz.geom) == fields(r.geom) and fields(lz.shape) == fields(r.shape)
    assert lz.info == (6, 128, 512, 1) and wgrad(mods, layer, lz).unfold
    # ... whose operand keeps its affine (write-out switched off): forward and weight gradient both on the layer's own geometry
    switch("MATERIALIZE_FOR_DMA", False)
    kept = forward(mods, layer, 4, 64, 2048, lazy=True)
    assert kept.write_out is None and kept.image == "gather" and fields(kept.geom) == (3, 3, 2, 1, 1, 128, 128)
    wk = wgrad(mods, layer, kept)
    assert not wk.unfold and wk.v_pitch == 1 and wk.shape.flags & L.IN_AFFINE and fields(wk.geom) == fields(layer.geom)
    switch("MATERIALIZE_FOR_DMA", True)
    # an odd fine width, or a pitch above the channels: no view
    assert forward(mods, layer, 4, 64, 2047).image == "gather" and forward(mods, layer, 4, 64, 2048, ld=256).image == "gather"
    switch("FOLD_STRIDED", False)
    layer = conv(E, 128, 128, 3, 2)  # (a fresh layer: the folded geometry is cached on it)
    r = forward(mods, layer, 4, 64, 2048)
    assert r.image == "gather" and fields(r.geom) == (3, 3, 2, 1, 1, 128, 128) and r.info == (1, 36, 4096, 1)
    w = wgrad(mods, layer, r)
    assert not w.unfold and w.v_pitch == 1 and fields(w.geom) == fields(layer.geom)


def test_conv_transpose_backward_data_on_the_folded_view(mods):
    L, E, R = mods
    layer = E.tap_layer(torch.nn.ConvTranspose2d(128, 256, (3, 8), stride=(1, 4), padding=(1, 2), bias=False))
    f = forward(mods, layer, 4, 64, 512)
    assert f.image == "scatter" and (f.own.Wu, f.own.Wv) == (512, 2048)
    d = dgrad(mods, layer, f)
    assert d.form == "folded" and d.image == "folded" and fields(d.geom) == (3, 3, 1, 1, 1, 128, 1024)
    assert (d.shape.Wu, d.shape.Wv, d.shape.ld_src) == (512, 512, 4 * 256) and d.info == (6, 128, 256, 1) and not d.zero_first
    w = wgrad(mods, layer, f)
    assert w.unfold and w.v_pitch == 4
    # a dOut whose pitch exceeds its channels: no view
    d = dgrad(mods, layer, f, dout_ld=512)
    assert d.form == "plain" and d.image == "gather" and fields(d.geom) == fields(layer.geom) and d.shape.ld_src == 512


def test_1x1_stride2_backward_data_into_the_even_columns(mods, switch):
    L, E, R = mods
    layer = conv(E, 128, 256, 1, 2)
    f = forward(mods, layer, 2, 8, 256)
    for accumulate in (False, True):
        d = dgrad(mods, layer, f, accumulate=accumulate)
        assert d.form == "even_columns" and d.image == "scatter" and fields(d.geom) == (1, 1, 1, 0, 0, 256, 128)
        assert (d.shape.Wu, d.shape.Wv, d.shape.ld_dst) == (128, 128, 2 * 128) and d.zero_first == (not accumulate)
        assert bool(d.shape.flags & L.OUT_ACCUM) == accumulate and d.bnb_rows == 0
    switch("FOLD_STRIDED", False)
    d = dgrad(mods, layer, f)
    assert d.form == "plain" and fields(d.geom) == fields(layer.geom) and not d.zero_first


# ---- the epilogue and the early release -----------------------------------------------------------------------------------------
def test_bnb_epilogue_rows(mods, switch):
    L, E, R = mods
    layer = conv(E, 128, 128, 3)
    f = forward(mods, layer, 4, 64, 2656, lazy=True, out_flags=L.OUT_STATS)
    d = dgrad(mods, layer, f, bn_operand=True)
    assert d.form == "plain" and d.bnb_rows == L.load().rv_tap_bnb_rows(layer.geom, d.shape, 1) > 0
    assert dgrad(mods, layer, f, bn_operand=True, accumulate=True).bnb_rows == 0 and dgrad(mods, layer, f).bnb_rows == 0
    switch("BNB_FUSE", False)
    assert dgrad(mods, layer, f, bn_operand=True).bnb_rows == 0


def test_early_release_of_the_weight_gradient(mods, switch):
    L, E, R = mods
    layer = conv(E, 128, 128, 3)
    ragged = dgrad(mods, layer, forward(mods, layer, 4, 64, 2656))
    assert ragged.info[0] == 6 and ragged.info[2:] == (1328, 1) and ragged.early  # 1328 / (256 * 6) = 0.865 < 0.9
    full = dgrad(mods, layer, forward(mods, layer, 1, 64, 2048))
    assert full.info[0] == 6 and full.info[2:] == (256, 1) and not full.early  # exactly one round
    switch("EARLY_WGRAD_FILL", 0.0)
    assert not dgrad(mods, layer, forward(mods, layer, 4, 64, 2656)).early
    switch("EARLY_WGRAD_FILL", 0.9)
    switch("OVERLAP_WGRAD", False)
    assert not dgrad(mods, layer, forward(mods, layer, 4, 64, 2656)).early


def test_without_generation_6(mods):
    """Every launch above under ``select(SEL_NO_GEN6)``: the same write-out and form decisions on the generation the planner then gives
    (its answers for 256 CUs, written out), and no early release.  Rows: forward (write_out, image, info), backward-data (form, info),
    weight gradient (unfold, generation)."""
    L, E, R = mods
    convT = E.tap_layer(torch.nn.ConvTranspose2d(128, 256, (3, 8), stride=(1, 4), padding=(1, 2), bias=False))
    todo = [
        (conv(E, 256, 256, 3), (4, 64, 2048), True, L.OUT_STATS, ("dma", "gather", (5, 256, 2048, 1)), ("plain", (5, 256, 2048, 1)), (False, 3)),
        (conv(E, 256, 256, 1), (4, 64, 2048), True, 0, ("pointwise", "gather", (7, 256, 256, 1)), ("plain", (7, 256, 256, 1)), (False, 3)),
        (conv(E, 128, 128, 1), (4, 64, 2048), True, 0, (None, "gather", (2, 2, 4096, 1)), ("plain", (7, 128, 256, 1)), (False, 2)),
        (conv(E, 128, 128, 3, 2), (4, 64, 2048), False, 0, (None, "folded", (5, 128, 1024, 1)), ("plain", (4, 128, 2048, 1)), (True, 3)),
        (conv(E, 128, 128, 3, 2), (4, 64, 2048), True, 0, ("folded", "folded", (5, 128, 1024, 1)), ("plain", (4, 128, 2048, 1)), (True, 3)),
        (convT, (4, 64, 512), False, 0, (None, "scatter", (5, 256, 2048, 1)), ("folded", (5, 128, 512, 1)), (True, 3)),
        (conv(E, 128, 256, 1, 2), (2, 8, 256), False, 0, (None, "gather", (1, 36, 32, 2)), ("even_columns", (2, 2, 16, 1)), (True, 3)),
        (conv(E, 128, 128, 3), (4, 64, 2656), False, 0, (None, "gather", (5, 128, 2656, 1)), ("plain", (5, 128, 2656, 1)), (False, 3)),
        (conv(E, 128, 128, 3), (1, 64, 2048), False, 0, (None, "gather", (5, 128, 512, 1)), ("plain", (5, 128, 512, 1)), (False, 3)),
    ]
    with L.select(L.SEL_NO_GEN6):
        for i, (layer, nhw, lazy, out_flags, want_f, want_d, want_w) in enumerate(todo):
            f = forward(mods, layer, *nhw, lazy=lazy, out_flags=out_flags)
            d = dgrad(mods, layer, f)
            w = wgrad(mods, layer, f)
            assert f.shape.flags & L.SEL_NO_GEN6 and d.shape.flags & L.SEL_NO_GEN6 and w.shape.flags & L.SEL_NO_GEN6, i
            assert (f.write_out, f.image, f.info) == want_f, (i, f)
            assert (d.form, d.info) == want_d and not d.early, (i, d)
            assert (w.unfold, w.generation) == want_w, (i, w)
    # (the hint is per call: outside the block generation 6 is back)
    assert forward(mods, todo[0][0], 4, 64, 2048, lazy=True, out_flags=L.OUT_STATS).info[0] == 6
