"""An independent float64 rotated IoU, the first-order error bound of the project's fp32 IoU arithmetic, and the pair families the
accuracy tests run (``tests/test_iou_ref_cpu.py``, ``tests/test_gpu_iou_geometry.py``).  NumPy and plain Python only.

THE REFERENCE works on the rectangle the kernel is handed, ``[x1, y1, x2, y2, ry]`` as exact fp32 values: centre
``((x1+x2)/2, (y1+y2)/2)``, extents ``(x2-x1, y2-y1)``, turned by ``ry`` about the centre; sin / cos of ``ry`` in float64.  It is NOT
the clip of ``csrc/nms_geom.h`` in another precision (that is ``waymo_eval_ref.iou_pair``): it collects the corners of each rectangle
that lie in the other (closed tests in that rectangle's own frame), adds the intersections of every edge of one with every edge of
the other, orders the points by angle about their mean and takes the shoelace area; fewer than 3 points is area 0.  Everything is
done in coordinates relative to the centre of the first rectangle, so the reference does not lose digits with range.

THE INPUTS lie on a grid: centres on multiples of ``GRID`` = 2^-15 m, lengths and widths on multiples of 2 ``GRID``, every coordinate
below 256 m.  Then ``x - l/2`` and ``x + l/2`` are exact in fp32, and the three conventions the entries take (``[x1, y1, x2, y2, ry]``,
mmcv's ``[cx, cy, w, h, angle]``, ``[x, y, z, l, w, h, yaw]``) hand the kernel the SAME rectangle: one reference serves them all.  (At
200 m the fp32 spacing is 2^-16 m, so the grid is two fp32 steps there: the inputs are as fine as fp32 allows.)  Heights and z are on
the grid too, so the overlap in z is exact.

THE BOUND ``tol`` is derived in :func:`tol`; ``C`` is a count of roundings, not a measurement.
"""

from __future__ import annotations

import functools
import math

import numpy as np

U24 = 2.0 ** -24  # the relative rounding error of one fp32 operation
C = 8             # roundings from an input to a vertex of the intersection (:func:`tol`)
GRID = 2.0 ** -15
DISTANCES = (0.0, 30.0, 75.0, 200.0)
N_PAIRS = 120     # per family and distance (at most 512; a multiple of every cycle length below: 2, 3, 4, 5, 6, 8)
_SIGNS = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))


# ----------------------------------------------------------------------------------------------------------------------
# float64 reference
# ----------------------------------------------------------------------------------------------------------------------
def _frame(r):
    x1, y1, x2, y2, ry = (float(v) for v in r)
    return 0.5 * (x1 + x2), 0.5 * (y1 + y2), 0.5 * (x2 - x1), 0.5 * (y2 - y1), math.cos(ry), math.sin(ry)


def _corners(cx, cy, hx, hy, c, s):
    return [(cx + (sx * hx) * c - (sy * hy) * s, cy + (sx * hx) * s + (sy * hy) * c) for sx, sy in _SIGNS]


def inter_area64(rect_a, rect_b) -> float:
    """Area of the intersection of two rectangles ``[x1, y1, x2, y2, ry]``; 0 where either has no area."""
    ax, ay, ahx, ahy, ac, as_ = _frame(rect_a)
    bx, by, bhx, bhy, bc, bs = _frame(rect_b)
    if not (ahx > 0 and ahy > 0 and bhx > 0 and bhy > 0):
        return 0.0
    ox, oy = bx - ax, by - ay  # (coordinates relative to the centre of A from here on)
    pa, pb = _corners(0.0, 0.0, ahx, ahy, ac, as_), _corners(ox, oy, bhx, bhy, bc, bs)
    # closed tests with a slack far below anything fp32 resolves: a corner ON the boundary counts, whatever float64 rounding does to
    # it (identical boxes: all 8 corners are on the boundary).  A point kept by the slack alone moves the area by <= eps * perimeter.
    eps = 1e-12 * (ahx + ahy + bhx + bhy)

    def inside(p, cx, cy, hx, hy, c, s):
        dx, dy = p[0] - cx, p[1] - cy
        return abs(dx * c + dy * s) <= hx + eps and abs(dy * c - dx * s) <= hy + eps

    pts = [p for p in pa if inside(p, ox, oy, bhx, bhy, bc, bs)] + [p for p in pb if inside(p, 0.0, 0.0, ahx, ahy, ac, as_)]
    for i in range(4):
        p, p2 = pa[i], pa[(i + 1) & 3]
        rx, ry = p2[0] - p[0], p2[1] - p[1]
        for j in range(4):
            q, q2 = pb[j], pb[(j + 1) & 3]
            sx, sy = q2[0] - q[0], q2[1] - q[1]
            den = rx * sy - ry * sx
            if abs(den) <= 1e-14 * math.hypot(rx, ry) * math.hypot(sx, sy):
                continue  # parallel: the ends of a common stretch are corners, collected above
            wx, wy = q[0] - p[0], q[1] - p[1]
            t, u = (wx * sy - wy * sx) / den, (wx * ry - wy * rx) / den
            if -1e-12 <= t <= 1.0 + 1e-12 and -1e-12 <= u <= 1.0 + 1e-12:
                pts.append((p[0] + t * rx, p[1] + t * ry))
    if len(pts) < 3:
        return 0.0
    mx, my = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
    rel = sorted(((p[0] - mx, p[1] - my) for p in pts), key=lambda p: math.atan2(p[1], p[0]))
    return 0.5 * abs(sum(p[0] * q[1] - p[1] * q[0] for p, q in zip(rel, rel[1:] + rel[:1])))


def _area(r) -> float:
    return (float(r[2]) - float(r[0])) * (float(r[3]) - float(r[1]))


def iou64(rect_a, rect_b) -> float:
    inter = inter_area64(rect_a, rect_b)
    uni = _area(rect_a) + _area(rect_b) - inter
    return inter / uni if inter > 0.0 and uni > 0.0 else 0.0


def rect64(box7):
    """``[x, y, z, l, w, h, yaw]`` -> ``[x1, y1, x2, y2, ry]`` in float64 (exact for boxes on the grid)."""
    x, y, _, l, w, _, yaw = (float(v) for v in box7)
    return [x - 0.5 * l, y - 0.5 * w, x + 0.5 * l, y + 0.5 * w, yaw]


def _dz(a, b) -> float:
    a, b = [float(v) for v in a], [float(v) for v in b]
    return max(0.0, min(a[2] + 0.5 * a[5], b[2] + 0.5 * b[5]) - max(a[2] - 0.5 * a[5], b[2] - 0.5 * b[5]))


def iou3d64(box_a, box_b) -> float:
    """3-D IoU of two boxes ``[x, y, z (centre), l, w, h, yaw]``: intersection area times the overlap in z, over the union volume."""
    va, vb = float(box_a[3]) * float(box_a[4]) * float(box_a[5]), float(box_b[3]) * float(box_b[4]) * float(box_b[5])
    if not (va > 0 and vb > 0):
        return 0.0
    inter = inter_area64(rect64(box_a), rect64(box_b)) * _dz(box_a, box_b)
    return inter / (va + vb - inter) if inter > 0.0 else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------
def _area_error(rect_a, rect_b) -> float:
    """``C * 2^-24 * M * (P_a + P_b)``: see :func:`tol`."""
    m, per = 0.0, 0.0
    for r in (rect_a, rect_b):
        cx, cy, hx, hy, c, s = _frame(r)
        m = max([m] + [max(abs(x), abs(y)) for x, y in _corners(cx, cy, hx, hy, c, s)])
        per += 4.0 * (abs(hx) + abs(hy))
    return C * U24 * m * per


def tol(rect_a, rect_b) -> float:
    """First-order bound of ``|fp32 IoU - exact IoU|``: ``C * 2^-24 * M * (P_a + P_b) / U + 4 * 2^-24``.

    ``M`` is the largest absolute corner coordinate of the two rectangles, ``P`` their perimeters, ``U`` the exact area of the union.
    A vertex of the intersection that is off by ``d`` moves the intersection area by at most ``d`` times the perimeter it lies on, and an
    error of the area goes into the IoU divided by the union.  Every rounding on the way to a vertex is at most ``2^-24`` times the
    magnitude of its result, which is at most ``M`` (the half extents and their products are below ``M`` too).  ``C = 8`` counts them:

    1. the centre ``(x1 + x2) * 0.5``;
    2. the half extent ``(x2 - x1) * 0.5``;
    3. the product ``dx * c`` (the fp32 rounding of sin / cos is counted here: it is relative to a factor of the product);
    4. the product ``dy * s``;
    5. their difference (or sum);
    6. the sum with the centre: a corner;
    7. ``t = dp / (dp - dq)`` of the clip, taken as one rounding of the point it places on the edge;
    8. the interpolation ``p + t * (q - p)``.

    The shoelace sum, the two areas, the union and the division are relative errors of the IoU itself (at most 1, or barely above): the
    ``4 * 2^-24`` at the end.  The count is not tuned to any device; the measured worst ratios are in DESIGN.md.  Where the union has
    no area (a box without area: the IoU is 0 by definition) only the additive term is left."""
    uni = _area(rect_a) + _area(rect_b) - inter_area64(rect_a, rect_b)
    return (_area_error(rect_a, rect_b) / uni if uni > 0.0 else 0.0) + 4.0 * U24


def tol3d(box_a, box_b) -> float:
    """The same bound carried through ``I * dz / (V_a + V_b - I * dz)``: the error of the area times the (exact: the inputs are on the
    grid) overlap in z, over the union volume, plus ``4 * 2^-24`` for the volumes, the product, the union and the division."""
    ra, rb = rect64(box_a), rect64(box_b)
    dz = _dz(box_a, box_b)
    va, vb = _area(ra) * float(box_a[5]), _area(rb) * float(box_b[5])
    uni = va + vb - inter_area64(ra, rb) * dz
    return (_area_error(ra, rb) * dz / uni if uni > 0.0 else 0.0) + 4.0 * U24


# ----------------------------------------------------------------------------------------------------------------------
# conventions
# ----------------------------------------------------------------------------------------------------------------------
def rects_of(boxes7) -> np.ndarray:
    """(n,7) fp32 boxes -> (n,5) fp32 ``[x1, y1, x2, y2, ry]``; raises if a box is off the grid (the conversion would round)."""
    b = np.asarray(boxes7, np.float32).astype(np.float64).reshape(-1, 7)
    r = np.stack([b[:, 0] - 0.5 * b[:, 3], b[:, 1] - 0.5 * b[:, 4], b[:, 0] + 0.5 * b[:, 3], b[:, 1] + 0.5 * b[:, 4], b[:, 6]], 1)
    r32 = r.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), r), "a box off the grid: its rectangle is not exact in fp32"
    mid, ext = (r32[:, :2] + r32[:, 2:4]) * np.float32(0.5), r32[:, 2:4] - r32[:, :2]  # (fp32, as the kernel forms them)
    assert np.array_equal(mid.astype(np.float64), b[:, :2]) and np.array_equal(ext.astype(np.float64), b[:, 3:5])
    return r32


def mmcv_of(boxes7) -> np.ndarray:
    """(n,7) -> (n,5) ``[cx, cy, w, h, angle]`` of ``mmcv.ops.box_iou_rotated`` (first extent along ``(cos a, sin a)``)."""
    b = np.asarray(boxes7, np.float32).reshape(-1, 7)
    return np.ascontiguousarray(b[:, [0, 1, 3, 4, 6]])


# ----------------------------------------------------------------------------------------------------------------------
# pair families
# ----------------------------------------------------------------------------------------------------------------------
def _q(v, step=GRID):
    return np.round(np.asarray(v, np.float64) / step) * step


def _boxes(x, y, l, w, yaw, g):
    """Boxes on the grid: z within 0.25 m of 0, heights 1.5 .. 2 m (every pair overlaps in z)."""
    n = len(x)
    b = np.stack([_q(x), _q(y), _q(g.uniform(-0.25, 0.25, n)), _q(np.broadcast_to(l, (n,)), 2 * GRID), _q(np.broadcast_to(w, (n,)), 2 * GRID),
                  _q(g.uniform(1.5, 2.0, n), 2 * GRID), np.broadcast_to(yaw, (n,))], 1)
    return b.astype(np.float32)


def _centres(g, n, dist, integer=False):
    bearing = g.uniform(-math.pi, math.pi, n)  # (at the distance, within 4 m: no pair sits at the origin itself)
    x, y = dist * np.cos(bearing) + g.uniform(-4, 4, n), dist * np.sin(bearing) + g.uniform(-4, 4, n)
    return (np.round(x), np.round(y)) if integer else (x, y)


def _jittered(g, n, dist, l, w, sigma_xy, sigma_yaw):
    x, y = _centres(g, n, dist)
    yaw = g.uniform(-math.pi, math.pi, n)
    a = _boxes(x, y, l, w, yaw, g)
    b = _boxes(x + g.normal(0, sigma_xy, n), y + g.normal(0, sigma_xy, n), l, w, yaw + g.normal(0, sigma_yaw, n), g)
    return a, b


def cars(seed, dist, n=N_PAIRS):
    return _jittered(np.random.default_rng(seed), n, dist, 4.5, 2.0, 0.4, 0.1)


def pedestrians(seed, dist, n=N_PAIRS):
    return _jittered(np.random.default_rng(seed), n, dist, 0.6, 0.6, 0.1, 0.3)


def trucks_parallel(seed, dist, n=N_PAIRS):
    """20 x 2.5, the second shifted by up to a few decimetres; yaw difference 0, 1e-6, 1e-4 in turn (before the fp32 rounding of the yaw)."""
    g = np.random.default_rng(seed)
    x, y = _centres(g, n, dist)
    yaw = g.uniform(-math.pi, math.pi, n)
    a = _boxes(x, y, 20.0, 2.5, yaw, g)
    b = _boxes(x + g.normal(0, 0.3, n), y + g.normal(0, 0.3, n), 20.0, 2.5, yaw + np.asarray([0.0, 1e-6, 1e-4])[np.arange(n) % 3], g)
    b[np.arange(n) % 3 == 0, 6] = a[np.arange(n) % 3 == 0, 6]  # difference 0: the same fp32 yaw
    return a, b


def _identical_boxes(g, n, dist, yaw, lmax=20.0):
    x, y = _centres(g, n, dist)
    return _boxes(x, y, g.uniform(0.3, lmax, n), g.uniform(0.3, 3.0, n), yaw, g)


def identical(seed, dist, n=N_PAIRS):
    """``b = a``; yaw 0, pi/2, -pi/2, pi and random in +-7 rad in turn; 0.3 .. 20 m by 0.3 .. 3 m."""
    g = np.random.default_rng(seed)
    k = np.arange(n) % 5
    yaw = np.where(k == 4, g.uniform(-7.0, 7.0, n), np.asarray([0.0, math.pi / 2, -math.pi / 2, math.pi, 0.0])[k])
    a = _identical_boxes(g, n, dist, yaw)
    return a, a.copy()


def identical_mod_2pi(seed, dist, n=N_PAIRS):
    """``b = a`` with the yaw a whole turn on, as ``atan2 + azimuth`` decodes it; the sizes of ``identical``.  fp32(yaw + 2 pi) is up to
    2.4e-7 rad off the whole turn, which moves the end of a box of length l by l/2 times that: the exact IoU of the pair is below 1 by
    about ``2.4e-7 * l / w`` (1.6e-5 for 20 x 0.3), which is at most a fifth of the pair's ``tol`` -- "within ``tol`` of 1" is a fair
    demand, and the reference is evaluated on the rounded yaw all the same."""
    g = np.random.default_rng(seed)
    a = _identical_boxes(g, n, dist, g.uniform(-math.pi, math.pi, n))
    b = a.copy()
    b[:, 6] = (a[:, 6].astype(np.float64) + 2.0 * math.pi).astype(np.float32)
    return a, b


_TURNS = (0.0, math.pi / 2, math.pi, -math.pi / 2)


def _turned(dx, dy, k):
    """(dx, dy) turned by k quarter turns: exact on integers."""
    for _ in range(k % 4):
        dx, dy = -dy, dx
    return dx, dy


def _lattice_pairs(seed, dist, n, offset):
    """4 x 2 boxes on integer centres: the second at ``offset`` in the frame of the first, both turned by k quarter turns (the fp32
    yaw is not an exact quarter turn: the reference sees the sliver that leaves)."""
    g = np.random.default_rng(seed)
    x, y = _centres(g, n, dist, integer=True)
    k = np.arange(n) % 4
    off = np.asarray([_turned(offset[0], offset[1], int(q)) for q in k], np.float64)
    yaw = np.asarray(_TURNS)[k]
    return _boxes(x, y, 4.0, 2.0, yaw, g), _boxes(x + off[:, 0], y + off[:, 1], 4.0, 2.0, yaw, g)


def shared_edge(seed, dist, n=N_PAIRS):
    """The short edge shared (even pairs) or the long edge (odd pairs); axis-aligned and in quarter turns; exact IoU 0 (or a sliver of
    the order of 1e-8 where the fp32 yaw of a quarter turn is off)."""
    a, b = _lattice_pairs(seed, dist, n, (4.0, 0.0))
    a2, b2 = _lattice_pairs(seed, dist, n, (0.0, 2.0))
    odd = (np.arange(n) // 4) % 2 == 1
    a[odd], b[odd] = a2[odd], b2[odd]
    return a, b


def touching_corner(seed, dist, n=N_PAIRS):
    return _lattice_pairs(seed, dist, n, (4.0, 2.0))


def contained(seed, dist, n=N_PAIRS):
    """A 1 .. 2 by 0.5 .. 1 box (circumradius <= 1.12) within 0.35 m of the centre of a 6 .. 10 by 3 .. 4 box (inradius >= 1.5)."""
    g = np.random.default_rng(seed)
    x, y = _centres(g, n, dist)
    a = _boxes(x, y, g.uniform(6, 10, n), g.uniform(3, 4, n), g.uniform(-math.pi, math.pi, n), g)
    b = _boxes(x + g.uniform(-0.25, 0.25, n), y + g.uniform(-0.25, 0.25, n), g.uniform(1, 2, n), g.uniform(0.5, 1, n), g.uniform(-7, 7, n), g)
    return a, b


def concentric_rot(seed, dist, n=N_PAIRS):
    """The same centre and size, turned by 45 and 90 degrees in turn."""
    g = np.random.default_rng(seed)
    x, y = _centres(g, n, dist)
    l, w, yaw = g.uniform(0.5, 10, n), g.uniform(0.5, 3, n), g.uniform(-math.pi, math.pi, n)
    l[::4] = w[::4]  # squares among them
    a = _boxes(x, y, l, w, yaw, g)
    b = a.copy()
    b[:, 6] = (a[:, 6].astype(np.float64) + np.where(np.arange(n) % 2 == 0, math.pi / 4, math.pi / 2)).astype(np.float32)
    return a, b


def thin(seed, dist, n=N_PAIRS):
    """4.5 x 0.05, shifted by centimetres across and decimetres along, turned by milliradians."""
    g = np.random.default_rng(seed)
    x, y = _centres(g, n, dist)
    yaw = g.uniform(-math.pi, math.pi, n)
    along, across = g.normal(0, 0.3, n), g.normal(0, 0.02, n)
    a = _boxes(x, y, 4.5, 0.05, yaw, g)
    b = _boxes(x + along * np.cos(yaw) - across * np.sin(yaw), y + along * np.sin(yaw) + across * np.cos(yaw), 4.5, 0.05, yaw + g.normal(0, 0.005, n), g)
    return a, b


def no_area(seed, dist, n=N_PAIRS):
    """Cars whose first box has l = 0 (even pairs) or w = 0 (odd pairs), and every fourth pair the second box too: IoU 0 by definition."""
    a, b = cars(seed, dist, n)
    a[0::2, 3], a[1::2, 4], b[0::4, 4] = 0.0, 0.0, 0.0
    return a, b


MARGINS = (-2e-3, -2e-4, 2e-4, 2e-3)


def circle_margin(seed, dist, n=N_PAIRS):
    """Corner to corner: the diagonals of the two boxes lie on one line and the centres are ``(r_a + r_b) * (1 + e)`` apart, ``e`` in
    ``MARGINS`` in turn (``r``: half the diagonal) -- the pairs closest to the bounding-circle exits that still (e < 0) overlap, by a
    square of diagonal ``-e (r_a + r_b)``, or (e > 0) do not.  Cars, pedestrians and trucks in turn.  :func:`circle_ratio` gives what the
    grid made of ``1 + e``."""
    g = np.random.default_rng(seed)
    x, y = _centres(g, n, dist)
    size = np.asarray([(4.5, 2.0), (0.6, 0.6), (20.0, 2.5)])[(np.arange(n) // 4) % 3]
    size = _q(size, 2 * GRID)
    r = 0.5 * np.hypot(size[:, 0], size[:, 1])
    e = np.asarray(MARGINS)[np.arange(n) % 4]
    phi = g.uniform(-math.pi, math.pi, n)
    alpha = np.arctan2(size[:, 1], size[:, 0])
    d = 2.0 * r * (1.0 + e)
    a = _boxes(x, y, size[:, 0], size[:, 1], phi - alpha, g)
    b = _boxes(x + d * np.cos(phi), y + d * np.sin(phi), size[:, 0], size[:, 1], phi + math.pi - alpha, g)
    ratio = circle_ratio(a, b)
    assert np.all(np.abs(ratio - (1.0 + e)) < 1e-4), "the grid moved a pair across its margin"
    return a, b


def circle_ratio(a, b) -> np.ndarray:
    """Centre distance over the sum of the circumradii, float64."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    reach = 0.5 * (np.hypot(a[:, 3], a[:, 4]) + np.hypot(b[:, 3], b[:, 4]))
    return np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]) / reach


FAMILIES = {f.__name__: f for f in (cars, pedestrians, trucks_parallel, identical, identical_mod_2pi, shared_edge, touching_corner, contained,
                                    concentric_rot, thin, no_area, circle_margin)}
# where the float64 clip (waymo_eval_ref.iou_pair) and this reference are both well conditioned
NON_DEGENERATE = ("cars", "pedestrians", "contained", "concentric_rot", "thin")


class Case:
    """One family at one distance: the boxes, the rectangles, and the float64 IoUs and bounds of the pairs ``(a[k], b[k])``."""

    def __init__(self, family: str, dist: float) -> None:
        self.family, self.dist = family, dist
        seed = 1000 * sorted(FAMILIES).index(family) + int(dist)
        self.a, self.b = FAMILIES[family](seed, dist)
        assert len(self.a) <= 512 and float(np.abs(np.concatenate([self.a, self.b])[:, :2]).max()) < 230.0
        self.ra, self.rb = rects_of(self.a), rects_of(self.b)
        pairs = list(zip(self.ra, self.rb))
        self.iou = np.asarray([iou64(p, q) for p, q in pairs])
        self.tol = np.asarray([tol(p, q) for p, q in pairs])
        self.iou3d = np.asarray([iou3d64(p, q) for p, q in zip(self.a, self.b)])
        self.tol3d = np.asarray([tol3d(p, q) for p, q in zip(self.a, self.b)])
        for v in (self.a, self.b, self.ra, self.rb, self.iou, self.tol, self.iou3d, self.tol3d):
            v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(family: str, dist: float) -> Case:
    """Computed once per process and shared; the arrays are read-only."""
    return Case(family, float(dist))


def all_cases():
    return [(f, d) for f in FAMILIES for d in DISTANCES]


# ----------------------------------------------------------------------------------------------------------------------
# what every IoU entry has to satisfy on a case (the CPU arithmetic and each device entry go through the same function)
# ----------------------------------------------------------------------------------------------------------------------
def fair_overlap(c: Case) -> np.ndarray:
    """``circle_margin`` pairs inside the circle whose overlap no rounding can remove: the overlap is a rectangle with the diagonal
    ``(1 - ratio) * (r_a + r_b)`` along the diagonal of the boxes; a disc of radius half its shorter side lies in both boxes, and each
    box's outline moves by at most ``C * 2^-24 * M``.  Where the radius is above twice that, the fp32 intersection cannot be empty."""
    a = c.a.astype(np.float64)
    ratio = circle_ratio(c.a, c.b)
    diag = np.hypot(a[:, 3], a[:, 4])
    depth = (1.0 - ratio) * diag
    short = depth * np.minimum(a[:, 3], a[:, 4]) / diag
    m = np.abs(np.concatenate([c.a[:, :2], c.b[:, :2]], 1)).max(1) + 0.5 * diag
    return (ratio < 1.0) & (0.5 * short > 2.0 * C * U24 * m)


def check_values(c: Case, got, who: str, three_d: bool = False) -> float:
    """Asserts what the accuracy statement says of ``got`` (n,) -- an entry's IoU of the pairs of ``c`` (its 3-D IoU under ``three_d``)
    -- and returns the worst ``error / tol``."""
    got = np.asarray(got).astype(np.float64).reshape(-1)
    want, bound = (c.iou3d, c.tol3d) if three_d else (c.iou, c.tol)
    tag = f"{who} {c.family} at {c.dist:g} m"
    err = np.abs(got - want)
    k = int(np.argmax(err / bound))
    assert np.all(err <= bound), f"{tag}: pair {k}: got {got[k]!r}, exact {want[k]!r}, error {err[k]:.3e} > tol {bound[k]:.3e}\n{c.a[k]}\n{c.b[k]}"
    assert np.all(got >= 0.0) and np.all(got <= 1.0 + bound), f"{tag}: outside [0, 1 + tol]: {got.min()!r} .. {got.max()!r}"
    if c.family in ("identical", "identical_mod_2pi"):
        assert np.all(np.abs(got - 1.0) <= bound), f"{tag}: an identical pair further than tol from 1: {np.abs(got - 1.0).max():.3e}"
    if c.family == "no_area":
        assert np.all(got == 0.0) and np.all(want == 0.0), f"{tag}: a pair without area with an IoU"
    if c.family == "circle_margin":
        outside = circle_ratio(c.a, c.b) > 1.0
        assert outside.sum() == len(got) // 2 and np.all(want[outside] == 0.0) and np.all(want[~outside] > 0.0)
        assert np.all(got[outside] == 0.0), f"{tag}: {int((got[outside] != 0).sum())} pairs with their bounding circles apart have an IoU"
        fair = fair_overlap(c)
        assert np.all(got[fair] > 0.0), f"{tag}: {int((got[fair] == 0).sum())} overlapping pairs just inside the bounding circle came out 0"
    return float(err[k] / bound[k])


def self_iou32(rects) -> np.ndarray:
    """What the IoU of a rectangle WITH ITSELF has to be, bit for bit.  Every corner of A lies on an edge line of B = A with a cross
    product that is exactly 0 (``(e1 - e0) x (e1 - e0)``: the same two products) and the other two corners lie well inside, so a clip
    with closed half-plane tests (``>=``) interpolates nothing and returns A's own four fp32 corners in their order; the area is their
    fp32 shoelace sum about corner 0 and the IoU is ``inter / (area + area - inter)``.  Only that much of the arithmetic is restated
    here (corners and shoelace, as ``csrc/nms_geom.h`` declares them): a clip that treats a boundary point as outside replaces corners
    by ``p + 1 * (q - p)``, which rounds wherever the coordinates change sign or magnitude, and shows up in the last bits."""
    r = np.asarray(rects, np.float32).reshape(-1, 5)
    half = np.float32(0.5)
    cx, cy, hx, hy = (r[:, 0] + r[:, 2]) * half, (r[:, 1] + r[:, 3]) * half, (r[:, 2] - r[:, 0]) * half, (r[:, 3] - r[:, 1]) * half
    s, c = np.sin(r[:, 4].astype(np.float64)).astype(np.float32), np.cos(r[:, 4].astype(np.float64)).astype(np.float32)
    px, py = [], []
    for sx, sy in _SIGNS:
        dx, dy = np.float32(sx) * hx, np.float32(sy) * hy
        px.append(cx + (dx * c - dy * s))
        py.append(cy + (dx * s + dy * c))
    twice = np.zeros(len(r), np.float32)
    for k in range(4):
        q = (k + 1) & 3
        twice = twice + ((px[k] - px[0]) * (py[q] - py[0]) - (py[k] - py[0]) * (px[q] - px[0]))
    inter = half * np.abs(twice)
    area = (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
    return (inter / (area + area - inter)).astype(np.float32)
