"""Host routes of a conv op: WHAT ``engine.ConvOp`` and ``engine_bwd.conv_backward`` launch, decided once per op, in one place."""
# Three frozen records -- FwdRoute, DgradRoute, WgradRoute -- made by pure functions of plain values (the layer's geometry, N / H / W,
# pixel pitches, padded channel counts, flag words, booleans; of a ``TapLayer`` only ``geom``, ``transposed``, ``fwd_form`` and
# ``fold_geom()`` are used).  Everything asked of the library is host-only (rv_tap_launch_info,
# rv_fold_geom through TapLayer.fold_geom, rv_tap_stats_rows, rv_tap_bnb_rows, rv_tap_wgrad_info): no
# tensor, no launch, no GPU.  The switches stay attributes of ``engine`` (tests and A/B tools flip them in-process) and are read here,
# when the decision is made; ``_lib.select`` / ``_lib.operand`` change the planner's answers the same way.  A route is computed per
# op and kept nowhere else: no staleness rule.

import ctypes
from collections import namedtuple

from . import _lib as L
from . import engine as E  # (only for its switches; engine itself imports this module where it uses it)

DMA_GENERATIONS = (4, 5, 6)  # the LDS-DMA tap-convs: operands stream global -> LDS past the registers, so they take PLAIN operands only


def _info(route) -> tuple:
    # (generation, variant, grid.x, grid.y) of the launch; asked now unless the decision already had to
    info = route.known or L.tap_launch_info(route.geom, route.shape, route.image == "scatter")
    if info is None:
        raise L.RvError(f"rv_tap_launch_info failed: {L.load().rv_last_error().decode()}")
    return info


# The records (immutable).  Common to the two tap launches:
#   geom, shape  what is launched: the layer's own geometry and shape, or those of a stride-1 view
#   image        weight image: gather / scatter / folded (a folded image is gathered)
#   known        the planner's answer for (geom, shape) when the decision needed one; ``info`` asks when it did not
# FwdRoute:   write_out  a folded BatchNorm operand is written out first: "dma" / "pointwise" / "folded", or None
#             own        the launch in the layer's own geometry (``ConvOp.shape``: what backward starts from)
#             rows       statistics rows (0 without OUT_STATS)
# DgradRoute: form       plain / folded / even_columns (no input gradient, or a fused form of it: no route)
#             zero_first even_columns: the odd columns of a destination that holds nothing yet
#             bnb_rows   rows of the rv_tap_data_grad_bnb epilogue; 0: the plain launch
#             early      the weight gradient is released BEFORE this launch (engine.EARLY_WGRAD_FILL)
# WgradRoute: v_pitch    multiplier of the pixel pitch of ``v`` (the stride on the folded view)
#             unfold     rv_unfold_weight_grad picks the layer's own entries out of the folded gradient
#             generation (profile name only) asked of rv_tap_wgrad_info when read
class FwdRoute(namedtuple("FwdRoute", "geom shape image known write_out own rows")):
    info = property(_info)


class DgradRoute(namedtuple("DgradRoute", "geom shape image known form zero_first bnb_rows early")):
    info = property(_info)


class WgradRoute(namedtuple("WgradRoute", "geom shape v_pitch unfold")):
    @property
    def generation(self) -> int:
        info = (ctypes.c_int32 * 4)()
        L.call("rv_tap_wgrad_info", self.geom, self.shape, info)
        return info[0]


def fold_geom_for(layer, wu: int, w: int, ld: int, cp: int):
    # THE folded-view condition: the stride-1 geometry of a strided layer over its fine tensor (width, pitch, stored channels), or None;
    # the fine tensor reads as (N, H, Wu, s * C): dense pixels, and a width of exactly s * Wu (an odd width keeps the generic kernel:
    # the view's row pitch is Wu * s * ld)
    gf = layer.fold_geom()  # (None for stride 1, a permuted weight, engine.FOLD_STRIDED off)
    return gf if gf is not None and ld == cp and w == layer.geom.stride_w * wu else None


def folded_gather(layer, n: int, h: int, wu: int, w: int, ld: int, cp: int, ld_dst: int, flags: int):
    # (geometry, shape, planner info) of a strided gather on the folded view of its source, when the planner gives that an LDS-DMA kernel
    gf = fold_geom_for(layer, wu, w, ld, cp)
    shape = L.TapShape(n, h, wu, wu, layer.geom.stride_w * ld, ld_dst, flags)
    info = L.tap_launch_info(gf, shape, False) if gf is not None else None
    return (gf, shape, info) if info is not None and info[0] in DMA_GENERATIONS else None


def forward_route(layer, n: int, h: int, w: int, ld: int, cp: int, operand_flags: int, ld_dst: int, out_flags: int) -> FwdRoute:
    """Forward of ``layer`` over an (n, h, w) source of pitch ``ld`` and ``cp`` stored channels."""
    # operand_flags: IN_AFFINE (| IN_RELU) when the operand is a folded BatchNorm, else 0; out_flags: every OUT_* flag of the launch
    # (OUT_BIAS: a bias or an eval fold)
    g, scatter = layer.geom, layer.transposed
    wu, wv = (w, w * g.stride_w) if scatter else (w // g.stride_w, w)
    write_out = view = known = None
    # Writing the operand out (engine.MATERIALIZE_FOR_DMA): asked of the launch WITHOUT the folded BatchNorm -- the same shape, operand flags
    # cleared, pitch of the written tensor.
    if operand_flags and E.MATERIALIZE_FOR_DMA and not out_flags & L.OUT_F32:
        plain = L.TapShape(n, h, wu, wv, cp, ld_dst, out_flags)
        if g.kh * g.kw > 1:  # (not 1x1 layers in general: there the extra pass costs what the faster kernel saves)
            known = L.tap_launch_info(g, plain, scatter)
            if known is not None and known[0] in DMA_GENERATIONS:
                write_out = "dma"
            elif not scatter:  # strided: the FOLDED form (forward and weight gradient) on the LDS-DMA kernels instead of the generic strided ones
                view = folded_gather(layer, n, h, wu, w, ld, cp, ld_dst, out_flags)  # (of the tensor as it is: dense, as the written one)
                write_out = "folded" if view is not None else None
        elif E.MATERIALIZE_FOR_POINTWISE and not out_flags & L.OUT_BIAS and cp in E.MATERIALIZE_POINTWISE_C:
            known = L.tap_launch_info(g, plain, scatter)  # (engine.MATERIALIZE_FOR_POINTWISE: the streaming GEMM is generation 7)
            write_out = "pointwise" if known is not None and known[0] == 7 else None
    in_flags, pitch = (0, cp) if write_out else (operand_flags, ld)
    own = L.TapShape(n, h, wu, wv, pitch, ld_dst, in_flags | out_flags)
    if view is None and in_flags == 0 and not scatter:
        view = folded_gather(layer, n, h, wu, w, pitch, cp, ld_dst, out_flags)
    if view is not None:
        geom, shape, known = view
    else:
        geom, shape, known = g, own, known if write_out else None
    rows = L.load().rv_tap_stats_rows(geom, shape, 1 if scatter else 0) if out_flags & L.OUT_STATS else 0
    if rows < 0:
        raise L.RvError("rv_tap_stats_rows: " + L.load().rv_last_error().decode())
    return FwdRoute(geom, shape, "folded" if view is not None else layer.fwd_form, known, write_out, own, rows)


def dgrad_route(layer, sp, dout_w: int, dout_ld: int, dout_cp: int, dst_w: int, dst_ld: int, dst_cp: int, accumulate: bool,
                bn_operand: bool, cus) -> DgradRoute:
    """Backward-data of ``layer`` (the opposite tap form on the same geometry) from ``sp`` = the forward's own shape."""
    # accumulate: the destination already holds a contribution; bn_operand: the layer's input is relu?(bn(y)) with batch statistics;
    # cus(): compute units of the device (called only when the early-release rule needs them)
    g, scatter = layer.geom, not layer.transposed
    shape = L.TapShape(sp.N, sp.H, sp.Wu, sp.Wv, dout_ld, dst_ld, L.OUT_ACCUM if accumulate else 0)
    form, geom, image, known = "plain", g, "scatter" if scatter else "gather", None
    view = None if scatter else folded_gather(layer, sp.N, sp.H, sp.Wu, dout_w, dout_ld, dout_cp, dst_ld, shape.flags)
    if view is not None:
        # backward-data of a ConvTranspose2d = a strided gather over dOut: stride-1 on the folded view
        form, image, (geom, shape, known) = "folded", "folded", view
    elif (E.FOLD_STRIDED and scatter and g.stride_w == 2 and g.kh == 1 and g.kw == 1 and g.pad_w == 0 and dst_ld == dst_cp
          and dst_w == 2 * sp.Wu):
        # backward-data of a 1x1 stride-2 conv: only the even columns receive anything -- a STRIDE-1 1x1 launch into the even-column
        # view of the gradient (pixel pitch 2 ld; the one-tap scatter image is the same bytes), odd columns zeroed unless the buffer
        # already holds another consumer's contribution
        form, geom = "even_columns", L.TapGeom(1, 1, 1, 0, 0, g.cu, g.cv)
        shape = L.TapShape(sp.N, sp.H, sp.Wu, sp.Wu, dout_ld, 2 * dst_ld, shape.flags)
    # first (often only) consumer of relu(bn(y)): this launch can form that BatchNorm's backward sums on the way out
    bnb = E.BNB_FUSE and form == "plain" and bn_operand and not accumulate
    rows = max(L.load().rv_tap_bnb_rows(g, shape, 1 if scatter else 0), 0) if bnb else 0
    early = False
    if E.OVERLAP_WGRAD and E.EARLY_WGRAD_FILL > 0:
        # a persistent backward-data launch whose LAST round of tiles fills only part of the chip (1328 tiles on 256 CUs: five full
        # rounds and 48 tiles): the weight gradient of the same layer -- it reads dOut and the layer input, both complete -- is
        # released on an event recorded BEFORE this launch instead of after it, so both are eligible at once.  Nothing orders the
        # two on the hardware queues: the intent is that the weight gradient's workgroups take CUs as the last round leaves them idle;
        # when they take some earlier, this launch's rounds stretch by the same amount.  Kept on the measurement alone: rv-waymo
        # -1.0 ms chained / -0.15 ms free-running, rv-av2 (no ragged launch) unchanged (profiles/r04_ab_notes.md, r05_ab_notes.md)
        known = known or L.tap_launch_info(geom, shape, scatter)
        if known is not None and known[0] == 6:
            tiles, n_cu = known[2] * known[3], cus()
            early = tiles / (n_cu * ((tiles + n_cu - 1) // n_cu)) < E.EARLY_WGRAD_FILL
    return DgradRoute(geom, shape, image, known, form, form == "even_columns" and not accumulate, rows, early)


def wgrad_route(layer, sp, in_flags: int, v_w: int, v_ld: int, v_cp: int) -> WgradRoute:
    """Weight gradient of ``layer``; ``v`` is its fine tensor, ``in_flags`` what is still folded into the layer input."""
    # strided layers: on the stride-1 FOLDED view of a plain fine tensor (wgrad3 instead of the generic kernel), then
    # rv_unfold_weight_grad picks the kernel's own entries out of the folded gradient
    gf = fold_geom_for(layer, sp.Wu, v_w, v_ld, v_cp) if in_flags == 0 else None
    if gf is not None:
        return WgradRoute(gf, L.TapShape(sp.N, sp.H, sp.Wu, sp.Wu, 0, 0, L.WGRAD_TORCH_LAYOUT), layer.geom.stride_w, True)
    return WgradRoute(layer.geom, L.TapShape(sp.N, sp.H, sp.Wu, sp.Wv, 0, 0, in_flags | L.WGRAD_TORCH_LAYOUT), 1, False)
