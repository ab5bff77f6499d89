"""``tests/iou_ref.py`` against closed forms and against the float64 clip of ``tests/waymo_eval_ref.py``; then the project's fp32 IoU
arithmetic on the CPU (``oracle/c/oracle.c`` through ``oracle.nms.pairwise_iou``, which the kernels equal bit for bit) against the
reference within ``tol``, on every pair family at 0, 30, 75 and 200 m.  The last is the condition that the families are fair inputs for
the device tests (``tests/test_gpu_iou_geometry.py``); the worst ``error / tol`` of each family is printed (``pytest -s``)."""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import iou_ref as R  # noqa: E402
import waymo_eval_ref as W  # noqa: E402

REL = 1e-12


def _rect(cx, cy, l, w, yaw):
    return [cx - l / 2, cy - w / 2, cx + l / 2, cy + w / 2, yaw]


def _close(got, want, scale=None):
    return abs(got - want) <= REL * (abs(want) if scale is None else scale)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_axis_aligned_overlap_is_the_product_of_the_interval_overlaps():
    g = np.random.default_rng(3)
    for _ in range(200):
        cx, cy, dx, dy = g.uniform(-50, 50), g.uniform(-50, 50), g.uniform(-3, 3), g.uniform(-3, 3)
        la, wa, lb, wb = g.uniform(0.5, 6, 4)
        a, b = _rect(cx, cy, la, wa, 0.0), _rect(cx + dx, cy + dy, lb, wb, 0.0)
        ox = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
        oy = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
        assert _close(R.inter_area64(a, b), ox * oy, la * wa)
        assert _close(R.inter_area64(b, a), ox * oy, la * wa)
        uni = la * wa + lb * wb - ox * oy
        assert _close(R.iou64(a, b), ox * oy / uni, 1.0)
    # the same boxes, both described a half turn on: the same rectangles
    a, b = _rect(1.0, 2.0, 4.0, 2.0, math.pi), _rect(2.0, 2.5, 4.0, 2.0, -math.pi)
    assert _close(R.inter_area64(a, b), 3.0 * 1.5)
    # a quarter turn swaps the roles of the extents
    assert _close(R.inter_area64(_rect(0, 0, 4, 2, math.pi / 2), _rect(0, 0, 4, 2, 0.0)), 4.0)


@pytest.mark.parametrize("theta", [1e-3, 0.2, math.pi / 6, math.pi / 4, 1.0, math.pi / 2 - 1e-3, 2.0, 3.0, -0.7, 5.5])
def test_concentric_squares(theta):
    """Two concentric squares of side s, one turned by theta: an octagon of area 2 s^2 / (1 + |sin| + |cos|)."""
    for s, cx, cy, base in ((1.0, 0.0, 0.0, 0.0), (0.6, 150.0, -130.0, 0.4), (7.5, -20.0, 33.0, -2.9)):
        want = 2.0 * s * s / (1.0 + abs(math.sin(theta)) + abs(math.cos(theta)))
        assert _close(R.inter_area64(_rect(cx, cy, s, s, base), _rect(cx, cy, s, s, base + theta)), want)
        assert _close(R.iou64(_rect(cx, cy, s, s, base), _rect(cx, cy, s, s, base + theta)), want / (2 * s * s - want))


def test_containment_is_the_smaller_area():
    g = np.random.default_rng(5)
    for _ in range(200):
        cx, cy = g.uniform(-200, 200, 2)
        l, w = g.uniform(1, 2), g.uniform(0.5, 1)
        big = _rect(cx, cy, g.uniform(6, 10), g.uniform(3, 4), g.uniform(-7, 7))
        small = _rect(cx + g.uniform(-0.25, 0.25), cy + g.uniform(-0.25, 0.25), l, w, g.uniform(-7, 7))
        assert _close(R.inter_area64(big, small), l * w) and _close(R.inter_area64(small, big), l * w)
    box = _rect(3.0, 4.0, 4.5, 2.0, 0.3)
    assert _close(R.inter_area64(box, box), 9.0) and _close(R.iou64(box, box), 1.0)
    assert _close(R.inter_area64(box, _rect(3.0, 4.0, 4.5, 2.0, 0.3 + 2 * math.pi)), 9.0)


@pytest.mark.parametrize("theta", [0.0, math.pi / 2, 0.3, -2.2, 4.0])
def test_disjoint_shared_edge_and_touching_corner_are_zero(theta):
    """4 x 2 boxes; the second at an offset given in the frame of the first (placed in float64: exact to 1e-16)."""
    c, s = math.cos(theta), math.sin(theta)
    for cx, cy in ((0.0, 0.0), (120.0, -160.0)):
        a = _rect(cx, cy, 4.0, 2.0, theta)
        for ox, oy in ((4.0, 0.0), (0.0, 2.0), (-4.0, 0.0), (4.0, 2.0), (-4.0, 2.0), (4.0, 1.0), (9.0, 0.0), (3.0, 7.0)):
            b = _rect(cx + ox * c - oy * s, cy + ox * s + oy * c, 4.0, 2.0, theta)
            assert R.inter_area64(a, b) <= REL * 8.0 and R.iou64(a, b) <= REL, (theta, ox, oy)
        # a corner of the second on the middle of an edge of the first, turned by 45 degrees against it
        r = math.hypot(2.0, 1.0)
        b = _rect(cx + (2.0 + r) * c, cy + (2.0 + r) * s, 4.0, 2.0, theta + math.atan2(1.0, 2.0))
        assert R.inter_area64(a, b) <= REL * 8.0
    assert R.inter_area64(_rect(0, 0, 0.0, 2.0, 0.0), _rect(0, 0, 4.0, 2.0, 0.0)) == 0.0
    assert R.iou64(_rect(0, 0, 4.0, 0.0, 0.0), _rect(0, 0, 4.0, 2.0, 0.0)) == 0.0


def test_iou3d_closed_forms():
    a = [10.0, 20.0, 0.5, 4.0, 2.0, 2.0, 0.0]
    b = [11.0, 20.0, 1.0, 4.0, 2.0, 2.0, 0.0]
    inter = 3.0 * 2.0 * 1.5
    assert _close(R.iou3d64(a, b), inter / (32.0 - inter))
    assert R.iou3d64(a, [11.0, 20.0, 2.5, 4.0, 2.0, 2.0, 0.0]) == 0.0  # touching in z
    assert R.iou3d64(a, [11.0, 20.0, 1.0, 4.0, 2.0, 0.0, 0.0]) == 0.0  # no volume
    assert _close(R.iou3d64(a, a), 1.0)


def test_tol_is_the_stated_formula():
    a, b = _rect(100.0, 0.0, 4.0, 2.0, 0.0), _rect(101.0, 0.0, 4.0, 2.0, 0.0)
    uni = 16.0 - 6.0
    assert _close(R.tol(a, b), 8 * 2.0 ** -24 * 103.0 * 24.0 / uni + 4 * 2.0 ** -24)
    a7, b7 = [100.0, 0.0, 0.0, 4.0, 2.0, 2.0, 0.0], [101.0, 0.0, 1.0, 4.0, 2.0, 2.0, 0.0]
    assert _close(R.tol3d(a7, b7), 8 * 2.0 ** -24 * 103.0 * 24.0 * 1.0 / (32.0 - 6.0) + 4 * 2.0 ** -24)
    assert R.tol(_rect(0, 0, 0.0, 2.0, 0.0), a) > 0.0 and R.C == 8


# ---- the families --------------------------------------------------------------------------------------------------------------------
def test_families_are_deterministic_on_the_grid_and_at_their_distance():
    for name, fam in R.FAMILIES.items():
        for d in R.DISTANCES:
            a, b = fam(7, d)
            a2, b2 = fam(7, d)
            assert np.array_equal(a, a2) and np.array_equal(b, b2) and len(a) == len(b) <= 512, name
            assert a.dtype == np.float32 and np.isfinite(a).all() and np.isfinite(b).all()
            R.rects_of(a), R.rects_of(b)  # raises off the grid
            r = np.hypot(a[:, 0], a[:, 1])
            assert np.all(np.abs(r - d) <= 6.5), (name, d)
    c = R.case("circle_margin", 200.0)
    ratio = R.circle_ratio(c.a, c.b)
    for k, e in enumerate(R.MARGINS):
        assert np.all(np.abs(ratio[k::4] - (1.0 + e)) < 1e-4)
    assert R.fair_overlap(R.case("circle_margin", 0.0)).sum() == R.N_PAIRS // 2  # at the origin every inside pair is a fair demand
    assert R.fair_overlap(c).sum() >= R.N_PAIRS // 4  # at 200 m the pairs 2e-3 inside are
    y = R.case("identical", 75.0).a[:, 6]
    assert float(np.abs(y).max()) > math.pi + 1.0  # yaw outside (-pi, pi]
    t = R.case("trucks_parallel", 75.0)
    dyaw = np.abs(t.b[:, 6].astype(np.float64) - t.a[:, 6])
    assert np.all(dyaw[0::3] == 0.0) and np.all(dyaw[1::3] < 2e-6) and dyaw[1::3].max() > 0 and np.all(np.abs(dyaw[2::3] - 1e-4) < 1e-6)


@pytest.mark.parametrize("family", R.NON_DEGENERATE)
def test_reference_agrees_with_the_float64_clip(family):
    """Two algorithms, one answer to 1e-12.  The clip works in the coordinates it is given and loses digits with range (1e-11 at 200 m);
    it gets each pair moved to the origin, which float64 does exactly for boxes on the grid."""
    for d in R.DISTANCES:
        c = R.case(family, d)
        worst = 0.0
        for k in range(len(c.a)):
            a, b = c.a[k].astype(np.float64), c.b[k].astype(np.float64)
            b[:2] -= a[:2]
            a[:2] = 0.0
            bev, full = W.iou_pair(a, b)
            worst = max(worst, abs(bev - c.iou[k]), abs(full - c.iou3d[k]))
        assert worst <= REL, (family, d, worst)


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_fp32_arithmetic_on_the_cpu_is_within_tol(family):
    from oracle import nms as onms

    ratios = []
    for d in R.DISTANCES:
        c = R.case(family, d)
        got = onms.pairwise_iou(c.ra, c.rb).diagonal()
        ratios.append(R.check_values(c, got, "oracle.c"))
        assert c.tol.min() >= 4 * R.U24 and (family == "no_area" or c.tol.max() < 0.01)
    print(f"oracle.c {family}: worst error / tol at {R.DISTANCES} m: " + ", ".join(f"{r:.3f}" for r in ratios))
    if family in ("cars", "pedestrians", "trucks_parallel", "thin", "identical"):  # the error grows with range: so does the bound
        c0, c3 = R.case(family, 0.0), R.case(family, 200.0)
        assert np.median(c3.tol) > 10 * np.median(c0.tol)


def test_the_clip_of_a_box_by_itself_returns_its_own_corners():
    """Identical pairs, bit for bit against ``iou_ref.self_iou32``: the half-plane tests are closed (``dp >= 0``).  With open tests the
    value stays within ``tol`` -- the corners come back as ``p + 1 * (q - p)`` -- and only the last bits tell, near the origin."""
    from oracle import nms as onms

    for d in R.DISTANCES:
        c = R.case("identical", d)
        got = onms.pairwise_iou(c.ra, c.rb).diagonal()
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), R.self_iou32(c.ra).view(np.uint32)), d
