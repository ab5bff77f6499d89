"""NumPy restatement of the declared Waymo range-image -> sweep semantics (``include/rv3d.h``), an independently written
inverse of it, and a synthetic frame generator.  The restatement takes a dtype: ``float64`` is the yardstick the kernels are tested
against, ``float32`` the TensorFlow-like reading (used only to document the distance between the two).  Nothing here reads the
reference tree; nothing here imports the package."""

from __future__ import annotations

import numpy as np

SWEEP_CHANNELS = ("range", "intensity", "elongation", "x", "y", "z")
TABLE_COLUMNS = ("x", "y", "z", "range", "intensity", "elongation")
WAYMO_FEATURES = ("elongation", "intensity", "range", "x", "y", "z")


def compute_inclination(inclination_min, inclination_max, height):
    r = np.arange(height, dtype=np.float64)
    return (r + 0.5) / height * (inclination_max - inclination_min) + inclination_min


def inclinations_by_row(height, beam_inclinations=None, beam_inclination_min=None, beam_inclination_max=None):
    if beam_inclinations is not None and len(beam_inclinations):
        return np.asarray(beam_inclinations, np.float64)[::-1].copy()
    return compute_inclination(beam_inclination_min, beam_inclination_max, height)[::-1].copy()


def _rot(axis, angle):
    """Elementary rotations, stacked over the leading shape of ``angle``."""
    c, s, o, z = np.cos(angle), np.sin(angle), np.ones_like(angle), np.zeros_like(angle)
    rows = {"x": [o, z, z, z, c, -s, z, s, c], "y": [c, z, s, z, o, z, -s, z, c], "z": [c, -s, z, s, c, z, z, z, o]}[axis]
    return np.stack(rows, -1).reshape(angle.shape + (3, 3))


def azimuths(extrinsic, width, dtype=np.float64):
    """(B, W): ``(2 (W - c - 0.5) / W - 1) pi - atan2(E[1,0], E[0,0])``."""
    E = np.asarray(extrinsic, dtype)
    correction = np.arctan2(E[:, 1, 0], E[:, 0, 0])
    c = np.arange(width, dtype=dtype)
    ratio = (dtype(width) - c - dtype(0.5)) / dtype(width)
    return ((dtype(2.0) * ratio - dtype(1.0)) * dtype(np.pi))[None, :] - correction[:, None]


def convert(range_image, extrinsic, inclination, pixel_pose=None, frame_pose=None, dtype=np.float64):
    """-> (sweep (B, H, W, 6) float32, num_pts (B,) int64, valid (B, H, W) bool, points (B, H, W, 3) in ``dtype`` before the final
    rounding -- garbage where not valid)."""
    ri = np.asarray(range_image, np.float32)
    B, H, W, _ = ri.shape
    E = np.asarray(extrinsic, dtype).reshape(B, 4, 4)
    incl = np.asarray(inclination, dtype).reshape(B, H)
    valid = (ri[..., 0] > 0) & (ri[..., 3] != np.float32(1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        rng = ri[..., 0].astype(dtype)
        az = azimuths(E, W, dtype)[:, None, :]
        ci, si = np.cos(incl)[:, :, None], np.sin(incl)[:, :, None]
        p = np.stack([rng * (np.cos(az) * ci), rng * (np.sin(az) * ci), rng * np.broadcast_to(si, rng.shape)], -1)
        p = np.einsum("bij,bhwj->bhwi", E[:, :3, :3], p) + E[:, None, None, :3, 3]
        if pixel_pose is not None:
            pp = np.asarray(pixel_pose, np.float32).astype(dtype)
            R = _rot("z", pp[..., 2]) @ _rot("y", pp[..., 1]) @ _rot("x", pp[..., 0])
            world = np.einsum("bhwij,bhwj->bhwi", R, p) + pp[..., 3:]
            V = np.linalg.inv(np.asarray(frame_pose, np.float64).reshape(B, 4, 4)).astype(dtype)  # formed in fp64, as the package does
            p = np.einsum("bij,bhwj->bhwi", V[:, :3, :3], world) + V[:, None, None, :3, 3]
        elif frame_pose is not None:
            raise ValueError("frame_pose without pixel_pose")
    sweep = np.zeros((B, H, W, 6), np.float32)
    sweep[..., :3] = np.where(valid[..., None], ri[..., :3], np.float32(0))
    sweep[..., 3:] = np.where(valid[..., None], p.astype(np.float32), np.float32(0))
    return sweep, valid.reshape(B, -1).sum(1).astype(np.int64), valid, p


def invert(points, extrinsic, pixel_pose=None, frame_pose=None):
    """The way back, written independently (SciPy rotations, transposes instead of the inverse matrix): vehicle frame at the frame's
    time -> world (frame pose) -> vehicle at the pixel's time (pixel pose transposed) -> sensor (extrinsic transposed) ->
    (range, azimuth, inclination) by norm, atan2, asin.  fp64."""
    from scipy.spatial.transform import Rotation

    p = np.asarray(points, np.float64)
    B, H, W, _ = p.shape
    E = np.asarray(extrinsic, np.float64).reshape(B, 4, 4)
    if pixel_pose is not None:
        F = np.asarray(frame_pose, np.float64).reshape(B, 4, 4)
        pp = np.asarray(pixel_pose, np.float32).astype(np.float64)
        out = np.empty_like(p)
        for b in range(B):
            world = p[b].reshape(-1, 3) @ F[b, :3, :3].T + F[b, :3, 3]
            rot = Rotation.from_euler("xyz", pp[b].reshape(-1, 6)[:, :3])  # extrinsic x, y, z = Rz(yaw) Ry(pitch) Rx(roll)
            out[b] = rot.inv().apply(world - pp[b].reshape(-1, 6)[:, 3:]).reshape(H, W, 3)
        p = out
    s = np.einsum("bji,bhwj->bhwi", E[:, :3, :3], p - E[:, None, None, :3, 3])
    rng = np.sqrt((s * s).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return rng, np.arctan2(s[..., 1], s[..., 0]), np.arcsin(s[..., 2] / rng)


def ulp32(x):
    """One fp32 unit in the last place of |x| (fp64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def make_frames(seed, B, H, W, offset=0.0, pixel_pose=True, beam_table=True):
    """Synthetic frames: ranges U(0.5, 75) m with ~10 % no-return (-1) pixels and a no-label-zone rectangle, an extrinsic with a yaw of
    some tenths of a radian, small roll / pitch and a lever arm, descending row inclinations, and the pixel poses of a vehicle at
    ~10 m/s with a small yaw rate over the 0.1 s spin, around a frame pose ``offset`` metres from the origin."""
    g = np.random.default_rng(seed)
    ri = np.empty((B, H, W, 4), np.float32)
    ri[..., 0] = g.uniform(0.5, 75.0, (B, H, W))
    ri[..., 0][g.random((B, H, W)) < 0.1] = -1.0
    ri[..., 1] = g.gamma(1.5, 0.4, (B, H, W))
    ri[..., 2] = g.uniform(0.0, 1.5, (B, H, W))
    ri[..., 3] = -1.0
    ri[:, H // 4:H // 2 + 1, W // 5:W // 3 + 1, 3] = 1.0
    ext = np.zeros((B, 4, 4), np.float64)
    fpose = np.zeros((B, 4, 4), np.float64)
    incl = np.empty((B, H), np.float64)
    pp = np.empty((B, H, W, 6), np.float32) if pixel_pose else None
    calib = []
    for b in range(B):
        yaw, pitch, roll = g.uniform(0.2, 0.6) * g.choice([-1.0, 1.0]), g.uniform(-0.02, 0.02), g.uniform(-0.02, 0.02)
        ext[b, :3, :3] = _rot("z", np.float64(yaw)) @ _rot("y", np.float64(pitch)) @ _rot("x", np.float64(roll))
        ext[b, :3, 3] = [1.43 + g.uniform(-0.05, 0.05), g.uniform(-0.05, 0.05), 2.184 + g.uniform(-0.05, 0.05)]
        ext[b, 3, 3] = 1.0
        if beam_table:  # ascending, non-uniform (denser towards the horizon), as the top lidar's table
            u = np.sort(g.random(H)) if H > 1 else np.array([0.5])
            table = -0.31 + 0.35 * u ** 0.7
            calib.append({"beam_inclinations": table, "beam_inclination_min": -0.31, "beam_inclination_max": 0.04})
        else:
            calib.append({"beam_inclinations": [], "beam_inclination_min": -0.31 + g.uniform(-0.01, 0.01), "beam_inclination_max": 0.04})
        incl[b] = inclinations_by_row(H, **calib[-1])
        yaw0, head = g.uniform(-np.pi, np.pi), g.uniform(-np.pi, np.pi)
        roll0, pitch0 = g.uniform(-0.03, 0.03), g.uniform(-0.03, 0.03)
        t0 = np.array([offset * np.cos(head), offset * np.sin(head), 12.0 + g.uniform(-5, 5)])
        fpose[b, :3, :3] = _rot("z", np.float64(yaw0)) @ _rot("y", np.float64(pitch0)) @ _rot("x", np.float64(roll0))
        fpose[b, :3, 3] = t0
        fpose[b, 3, 3] = 1.0
        if pixel_pose:
            t = ((np.arange(W) + 0.5) / W - 0.5) * 0.1  # seconds from the frame's timestamp, column by column
            t = t[None, :] + g.normal(0, 1e-5, (H, W))
            rate, speed = g.uniform(-0.2, 0.2), g.uniform(8.0, 12.0)
            pp[b, ..., 0] = roll0 + 0.01 * t
            pp[b, ..., 1] = pitch0 - 0.01 * t
            pp[b, ..., 2] = yaw0 + rate * t
            pp[b, ..., 3] = t0[0] + speed * t * np.cos(yaw0)
            pp[b, ..., 4] = t0[1] + speed * t * np.sin(yaw0)
            pp[b, ..., 5] = t0[2] + 0.05 * t
    return {"range_image": ri, "extrinsic": ext, "inclination": incl, "pixel_pose": pp, "frame_pose": fpose if pixel_pose else None,
            "calibration": calib}


def make_labels(sweep, valid, g, n=6):
    """A few labels centred on valid pixels of one frame's sweep (H, W, 6): the columns ``labels_to_annotations`` takes."""
    rows, cols = np.nonzero(valid)
    pick = g.choice(len(rows), size=n, replace=False)
    centre = sweep[rows[pick], cols[pick], 3:].astype(np.float64)
    kinds = np.array([1, 2, 4, 1, 3, 0, 1, 2][:n])  # VEHICLE, PEDESTRIAN, CYCLIST, VEHICLE, SIGN, UNKNOWN ...
    size = {0: (1, 1, 1), 1: (4.6, 2.0, 1.7), 2: (0.9, 0.8, 1.8), 3: (0.3, 0.3, 2.0), 4: (1.8, 0.8, 1.7)}
    dims = np.array([size[int(k)] for k in kinds], np.float64)
    return {"type": kinds, "center_x": centre[:, 0], "center_y": centre[:, 1], "center_z": centre[:, 2], "length": dims[:, 0], "width": dims[:, 1],
            "height": dims[:, 2], "heading": g.uniform(-np.pi, np.pi, n), "num_lidar_points_in_box": g.integers(1, 40, n),
            "detection_difficulty_level": g.integers(0, 3, n), "id": [f"obj{i}" for i in range(n)]}
