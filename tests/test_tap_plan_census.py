"""The tap-conv dispatcher's decisions at 256 compute units, pinned: for a census of calls, what ``rv_tap_launch_info`` (kernel generation,
variant, grid), ``rv_tap_stats_rows`` and ``rv_tap_bnb_rows`` answer -- return codes and error strings included -- must equal the recorded
answers in ``tests/golden/tap_plan_census.json``.  The planning entry points launch nothing and run without a device (they then plan for
256 compute units, an MI355X's count), so a change of the selection order, of an eligibility rule or of a grid / partial-row formula shows
up here, by call, before anything runs on a GPU.

The census: every conv geometry of the four shipped models (rv-av2 and base-av2 at 64 x 2048, rv-waymo and base-waymo at 64 x 2656, batch
4; the folded stride-1 views of their strided layers are geometries of their own) at every resolution of the backbone, in gather and
scatter form, under the epilogue / operand flags and the ``RV_SEL_*`` hints the engine and the tests use; a second channel stride; the
crops of the exact-integer kernel tests; and calls that must fail.

``python tests/test_tap_plan_census.py <librv3d_hip.so>`` rewrites the fixture from that library (do it from the commit BEFORE a change of
the dispatcher that is meant to keep its decisions, on a box without a GPU or with an MI355X)."""

from __future__ import annotations

import ctypes
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tap_plan_census.json")

IN_AFFINE, IN_RELU, OUT_F32, OUT_BIAS, OUT_STATS, OUT_ACCUM, OUT_RELU, OUT_RES_RELU = 1, 2, 4, 8, 16, 32, 64, 256
SMALL, SMALL6, NO6, NO5, NO_PW, NO_PW_BWD = (1 << b for b in range(20, 26))

# (kh, kw, stride_w, pad_h, pad_w, cu, cv) of every Conv2d / ConvTranspose2d of the models (cu: the coarse side's channels)
AV2 = [(1, 1, 1, 0, 0, 8, 512), (1, 1, 1, 0, 0, 26, 512), (1, 1, 1, 0, 0, 128, 128), (1, 1, 1, 0, 0, 256, 3), (1, 1, 1, 0, 0, 256, 5),
       (1, 1, 1, 0, 0, 256, 256), (1, 1, 1, 0, 0, 256, 2304), (1, 1, 2, 0, 0, 128, 128), (1, 1, 2, 0, 0, 128, 256), (3, 3, 1, 1, 1, 128, 128),
       (3, 3, 1, 1, 1, 128, 256), (3, 3, 1, 1, 1, 256, 256), (3, 3, 1, 1, 1, 512, 512), (3, 3, 2, 1, 1, 128, 128), (3, 4, 2, 1, 1, 128, 128),
       (3, 4, 2, 1, 1, 128, 256), (3, 8, 4, 1, 2, 128, 128), (3, 8, 4, 1, 2, 128, 256),
       # folded stride-1 views (rv_fold_geom) of the strided layers
       (1, 1, 1, 0, 0, 128, 512), (3, 2, 1, 1, 1, 128, 256), (3, 3, 1, 1, 1, 128, 512), (3, 3, 1, 1, 1, 128, 1024)]
WAYMO = [(1, 1, 1, 0, 0, 3, 256), (1, 1, 1, 0, 0, 8, 256), (1, 1, 1, 0, 0, 128, 3), (1, 1, 1, 0, 0, 128, 6), (1, 1, 1, 0, 0, 128, 128),
         (1, 1, 1, 0, 0, 128, 1152), (1, 1, 2, 0, 0, 128, 128), (3, 3, 1, 1, 1, 128, 128), (3, 3, 1, 1, 1, 256, 256), (3, 3, 2, 1, 1, 128, 128),
         (3, 4, 2, 1, 1, 128, 128), (3, 8, 4, 1, 2, 128, 128),
         (1, 1, 1, 0, 0, 128, 256), (3, 2, 1, 1, 1, 128, 256), (3, 3, 1, 1, 1, 128, 256), (3, 3, 1, 1, 1, 128, 512)]
BASE = [(1, 1, 1, 0, 0, 8, 128), (1, 1, 1, 0, 0, 26, 128), (1, 1, 1, 0, 0, 3, 128), (1, 1, 1, 0, 0, 64, 5), (1, 1, 1, 0, 0, 64, 6),
        (1, 1, 1, 0, 0, 64, 64), (1, 1, 1, 0, 0, 128, 128), (1, 1, 2, 0, 0, 64, 64), (1, 1, 2, 0, 0, 128, 64), (1, 1, 2, 0, 0, 128, 128),
        (3, 3, 1, 1, 1, 64, 64), (3, 3, 1, 1, 1, 128, 64), (3, 3, 1, 1, 1, 128, 128), (3, 3, 2, 1, 1, 64, 64), (3, 3, 2, 1, 1, 128, 128),
        (3, 4, 2, 1, 1, 64, 64), (3, 4, 2, 1, 1, 128, 64), (3, 8, 4, 1, 2, 128, 64), (3, 8, 4, 1, 2, 128, 128),
        (1, 1, 1, 0, 0, 64, 128), (1, 1, 1, 0, 0, 128, 256), (3, 2, 1, 1, 1, 64, 128), (3, 2, 1, 1, 1, 128, 256), (3, 3, 1, 1, 1, 64, 128),
        (3, 3, 1, 1, 1, 128, 256), (3, 3, 1, 1, 1, 128, 512)]
MODEL_FLAGS = [0, OUT_STATS, OUT_ACCUM, OUT_F32, OUT_BIAS | OUT_RELU, IN_AFFINE | IN_RELU, IN_AFFINE | IN_RELU | OUT_STATS,
               SMALL, SMALL6, NO6, NO5, NO_PW, NO_PW_BWD, SMALL | SMALL6, SMALL | NO6, NO5 | NO_PW, SMALL | NO5 | NO_PW, OUT_STATS | NO5]
# crops of tests/test_gpu_tapconv{2,4,5,6}.py and test_gpu_pointwise.py: (geometry, N, H, Wu)
CROPS = [((3, 3, 1, 1, 1, co, ci), n, h, w) for ci, co, n, h, w in
         [(64, 256, 4, 30, 520), (128, 512, 2, 64, 256), (192, 256, 4, 17, 1030), (64, 128, 4, 30, 520), (128, 384, 3, 32, 300), (512, 256, 1, 64, 288),
          (64, 256, 8, 8, 32), (128, 128, 2, 64, 256), (320, 128, 3, 17, 1030), (32, 128, 4, 30, 520), (96, 128, 4, 17, 1030), (512, 512, 1, 64, 288),
          (64, 128, 8, 16, 32), (320, 128, 3, 33, 1030), (128, 384, 1, 16, 96), (512, 512, 4, 64, 1024), (64, 256, 2, 24, 200), (64, 512, 1, 17, 96)]] + \
        [((1, 1, 1, 0, 0, co, ci), n, h, w) for ci, co, n, h, w in
         [(256, 256, 4, 32, 520), (64, 512, 2, 64, 300), (576, 256, 2, 33, 1000), (128, 128, 4, 32, 520), (128, 128, 2, 8, 2656), (128, 128, 1, 16, 333),
          (256, 256, 1, 8, 520), (256, 2304, 1, 16, 512)]] + \
        [((kh, kw, 1, (kh - 1) // 2, (kw - 1) // 2, 256, 128), 2, 24, 200) for kh, kw in [(3, 1), (1, 3), (3, 2)]] + \
        [((3, 4, 2, 1, 1, ci, co), n, h, w) for ci in (64, 128) for co in (256, 128) for n, h, w in [(4, 16, 512), (3, 21, 600)]] + \
        [((3, 8, 4, 1, 2, ci, co), n, h, w) for ci in (64, 128) for co in (256, 128) for n, h, w in [(4, 16, 256), (4, 16, 300)]]
CROP_FLAGS = [0, SMALL, SMALL | SMALL6, SMALL | NO6, SMALL | NO5, SMALL | OUT_STATS, SMALL | SMALL6 | OUT_ACCUM, SMALL | SMALL6 | OUT_BIAS]


def pad32(c: int) -> int:
    return (c + 31) & ~31


def census():
    """The calls, in a fixed order: (geometry, (N, H, Wu, Wv, ld_src, ld_dst, flags), scatter)."""
    calls = []

    def both_forms(geom, n, h, wu, flags, ld_scale=1):
        cu, cv = pad32(geom[5]), pad32(geom[6])
        for scatter in (0, 1):
            ld_src, ld_dst = (cu, cv) if scatter else (cv, cu)
            calls.append((geom, (n, h, wu, wu * geom[2], ld_src * ld_scale, ld_dst * ld_scale, flags), scatter))

    for width, geoms in ((2048, AV2 + BASE), (2656, WAYMO + BASE)):
        for geom in geoms:
            for level in (1, 2, 4, 8):
                if level < geom[2]:  # (the fine side of a strided layer is at most the full width)
                    continue
                for flags in MODEL_FLAGS:
                    both_forms(geom, 4, 64, width // level, flags)
                both_forms(geom, 4, 64, width // level, 0, ld_scale=2)  # written into / read from a channel slice of a wider tensor
                both_forms(geom, 4, 64, width // level, OUT_STATS, ld_scale=2)
    for geom, n, h, wu in CROPS:
        for flags in CROP_FLAGS:
            both_forms(geom, n, h, wu, flags)
    # calls that must fail
    g3 = (3, 3, 1, 1, 1, 128, 128)
    calls.append((g3, (4, 64, 512, 1024, 128, 128, 0), 0))                      # Wv != Wu * stride_w
    calls.append(((3, 3, 3, 1, 1, 128, 128), (4, 64, 512, 1536, 128, 128, 0), 0))  # stride 3
    calls.append((g3, (4, 64, 512, 512, 96, 128, 0), 0))                        # channel stride below the padded width
    calls.append((g3, (4, 64, 512, 512, 128, 132, 0), 1))                       # channel stride not a multiple of 8
    calls.append((g3, (0, 64, 512, 512, 128, 128, 0), 0))                       # empty tensor
    calls.append((g3, (4, 64, 512, 512, 128, 128, OUT_F32 | OUT_ACCUM), 0))     # accumulate into an fp32 destination
    calls.append(((5, 5, 1, 2, 2, 128, 128), (4, 64, 512, 512, 128, 128, 0), 0))  # 25 taps
    calls.append(((3, 8, 1, 1, 3, 32, 32), (1, 4, 64, 64, 32, 32, 0), 0))          # (a wide kernel on the generic path)
    return calls


def answers(handle):
    """One string per call: "rc info[0..3] | stats_rows | bnb_rows | error strings of the calls that failed"."""
    from range_view_3d_detection_amd._lib import TapGeom as _Geom, TapShape as _Shape  # (the typed binding takes no other struct)

    handle.rv_last_error.restype = ctypes.c_char_p
    out = []
    for geom, shape, scatter in census():
        g, s, info = _Geom(*geom), _Shape(*shape), (ctypes.c_int32 * 4)(-1, -1, -1, -1)
        errs = []
        rc = handle.rv_tap_launch_info(ctypes.byref(g), ctypes.byref(s), scatter, info)
        if rc != 0:
            errs.append(handle.rv_last_error().decode())
        rows = handle.rv_tap_stats_rows(ctypes.byref(g), ctypes.byref(s), scatter)
        if rows < 0:
            errs.append(handle.rv_last_error().decode())
        bnb = handle.rv_tap_bnb_rows(ctypes.byref(g), ctypes.byref(s), scatter)
        if bnb < 0:
            errs.append(handle.rv_last_error().decode())
        out.append(f"{rc} {list(info)} | {rows} | {bnb} | {' / '.join(errs)}")
    return out


@pytest.mark.parametrize("tag", ["bf16", "f16"])  # (both builds of the library plan alike)
def test_tap_plans_equal_the_recorded_census(tag):
    from range_view_3d_detection_amd import _lib

    rec = json.load(open(FIXTURE))
    got = answers(_lib.load(tag))
    want = [rec["answers"][i] for i in rec["index"]]
    assert len(got) == len(want) == len(census())
    wrong = [(call, g, w) for call, g, w in zip(census(), got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])
    # the census reaches every generation, the launches without fused BatchNorm-backward sums, and every kind of rejection
    gens = {a.split()[1].strip("[,") for a in got if a.startswith("0 ")}
    assert gens == {"1", "2", "4", "5", "6", "7"}, gens
    assert any(a.split(" | ")[2] == "0" for a in got) and any(int(a.split(" | ")[2]) > 0 for a in got)
    assert len({a.split(" | ")[3] for a in got if not a.startswith("0 ")}) >= 6


if __name__ == "__main__":
    got = answers(ctypes.CDLL(sys.argv[1]))
    uniq = sorted(set(got))
    pos = {a: i for i, a in enumerate(uniq)}
    with open(FIXTURE, "w") as f:
        json.dump({"compute_units": 256, "answers": uniq, "index": [pos[a] for a in got]}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(got)} calls, {len(uniq)} distinct answers -> {FIXTURE}")
