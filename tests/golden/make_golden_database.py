"""Fixtures for the object-database paste and the mid-chain ``point_dropout``: ``tests/golden/database/{paste,chain}.npz``.

Runs the REFERENCE's own ``sample_database`` / ``_intersection_test`` (``prototype/loader.py:708-789``), ``DataLoader._load_db``
(``:290-294``), ``DataLoader.apply_augmentations`` (``:514-549``) and ``DataLoader.__getitem__`` (``:568-705``) on the CPU, over the polars
stand-in of ``_ref_stubs.py`` extended HERE with what ``sample_database`` touches: ``sample`` (a RECORDED permutation -- polars' own
generator cannot be reproduced), ``concat``, ``read_ipc``, ``unique`` (``keep="first"``), ``rows``, ``partition_by``, ``to_series``.
``mmcv.ops.box_iou_rotated`` (absent here) is bound to a stand-in with mmcv's signature over ``oracle.nms.pairwise_iou``, as
``make_golden_assignment.py`` does.  ANGLE CONVENTION: mmcv's box ``(cx, cy, w, h, a)`` has its first extent along ``(cos a, sin a)`` in
the coordinates it is given (its "clockwise" refers to image coordinates, y pointing down), so the rectangle is
``[cx - w/2, cy - h/2, cx + w/2, cy + h/2, ry = +a]``.  Only the SIGN of the IoU is used: the stand-in asserts that every IoU is either 0
or above 1e-3 and that the sign pattern is the same with ``ry = -a``, so no fixture depends on the convention or on hairline contact.

A tiny database (13 rows, one of them with ``num_interior_pts == 0``) is written into a temporary directory in the reference's layout
(``db.feather`` + ``train/<category>/<row_nr>.feather``); its content is stored in ``paste.npz`` (``db/...``) so that the tests rebuild it.

``paste.npz`` -- ``sample_database`` + the join and sort of ``__getitem__`` (``:699-704``) on an 8 x 64 sweep:
* ``mixed``  a sample hitting a scene box (A); two samples hitting each other, both go (B, C); two samples sharing pixels without BEV
             overlap, the nearer wins per pixel (D in front of E); a sample fully hidden by nearer ones, removed from the annotations (G);
             a database point at the origin (mask False there, D); ``num_samples`` larger than the category (BUS: 5 of 3); a category
             outside ``tasks`` (BOLLARD: pasted, no annotation row);
* ``none``   a draw with no survivor.  Real polars refuses ``pl.concat([])``; the stand-in's empty frame carries the reference's code
             through: nothing is pasted, ``range_view *= range_mask`` still runs, the annotations stay;
* ``no_annotations``  a sweep without scene boxes; a degenerate sample (width 0: IoU with itself 0) goes (T).
``chain.npz`` -- ``apply_augmentations`` with ``point_dropout`` second (``second``), last (``last``) and followed by translation then scale
(``t_then_s``: a dropped pixel gets xyz = s t and a POSITIVE range), unpadded; and ``e2e``: ``__getitem__`` with ``enable_database``,
a chain with a mid-chain dropout, and the padding -- the database draw there is ``random.sample`` (recorded by the stand-in's ``sample``).

Reproducible byte for byte: every input lies on a grid that is exact in fp32; ``paste.npz`` holds copies and products with 0 / 1 only.
"""

from __future__ import annotations

import math
import os
import random
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stubs and imports the reference)
import _ref_stubs  # noqa: E402
from _ref_stubs import _PlFrame, _PlSeries  # noqa: E402
from make_golden import DictConfig, ListConfig, npy  # noqa: E402

import polars as pl  # noqa: E402  (stub)
import pyarrow as pa  # noqa: E402
import pyarrow.feather as feather  # noqa: E402
from torchbox3d.prototype import loader as ref_loader  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import nms as onms  # noqa: E402

OUT_DIR = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "database")
H, W = 8, 64
NAMES = ["intensity", "range", "x", "y", "z"]
BOX = ("tx_m", "ty_m", "tz_m", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz")
TASKS = {0: ["REGULAR_VEHICLE", "BUS"], 1: ["PEDESTRIAN"]}
RECORDED: list = []  # positions for the next ``DataFrame.sample`` calls (None: random.sample)
LAST_DRAWS: list = []


# ---- the polars stand-in, extended with what sample_database touches ----------------------------------------------------------------
class _Empty:
    """What the stand-in's ``concat([])`` returns: a frame without rows that answers the calls ``sample_database`` makes on it."""

    def __init__(self, n_cols: int = 0) -> None:
        self.n_cols = n_cols

    def sort(self, *_a, **_k):
        return self

    def unique(self, *_a, **_k):
        return self

    def select(self, columns):
        return _Empty(len(_ref_stubs._names_of(columns)))

    def to_series(self):
        return np.zeros(0, dtype=np.int64)

    def to_numpy(self, writable: bool = False):
        return np.zeros((0, self.n_cols), dtype=np.float32 if self.n_cols != 1 else np.int64)


def _sample(self, n):
    pos = RECORDED.pop(0) if RECORDED else None
    if pos is None:
        pos = random.sample(range(self.shape[0]), n)
    assert len(pos) == n and len(set(pos)) == n
    LAST_DRAWS.append([int(self._data["row_nr"][p]) for p in pos])
    return self[np.asarray(pos, dtype=np.int64)]


def _concat(frames):
    frames = list(frames)
    if not frames:
        return _Empty()
    cols = frames[0].columns
    assert all(sorted(f.columns) == sorted(cols) for f in frames), [f.columns for f in frames]
    return _PlFrame({c: np.concatenate([np.asarray(f._data[c]) for f in frames]) for c in cols})


def _unique(self, subset=None, keep="any", **_):
    if subset is None:
        assert len(self._data) == 1
        (k, v), = self._data.items()
        return _PlFrame({k: np.unique(v)})
    assert keep == "first"
    _, first = np.unique(self._data[subset], return_index=True)
    return self[np.sort(first)]


def _partition_by(self, by, as_dict=False):
    assert as_dict
    keys = self._data[by]
    out = {}
    for k in dict.fromkeys(keys.tolist()):  # first-appearance order, rows in file order
        out[k] = self[np.nonzero(keys == k)[0]]
    return out


_PlFrame.sample = _sample
_PlFrame.unique = _unique
_PlFrame.partition_by = _partition_by
_PlFrame.rows = lambda self: [tuple(v[i].item() if hasattr(v[i], "item") else v[i] for v in self._data.values()) for i in range(self.shape[0])]
_PlFrame.to_series = lambda self: next(iter(self._data.values()))
pl.concat = _concat
pl.read_ipc = _ref_stubs._pl_scan_ipc
pl.scan_ipc = _ref_stubs._pl_scan_ipc


def box_iou_rotated(bboxes1, bboxes2, mode="iou", aligned=False, clockwise=True):
    """``mmcv.ops.box_iou_rotated``: boxes ``(cx, cy, w, h, angle in radians)``, fp32 (see the module docstring for the convention)."""
    assert mode == "iou" and not aligned and bboxes1.dtype == torch.float32 and bboxes2.dtype == torch.float32

    def rect(b, sign):
        b = b.detach().numpy().astype(np.float32).reshape(-1, 5)
        hw, hh = np.float32(0.5) * b[:, 2], np.float32(0.5) * b[:, 3]
        return np.stack([b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh, np.float32(sign) * b[:, 4]], axis=1)

    if bboxes1.shape[0] == 0 or bboxes2.shape[0] == 0:
        return torch.zeros((bboxes1.shape[0], bboxes2.shape[0]), dtype=torch.float32)
    iou = onms.pairwise_iou(rect(bboxes1, 1), rect(bboxes2, 1))
    other = onms.pairwise_iou(rect(bboxes1, -1), rect(bboxes2, -1))
    assert ((iou == 0) | (iou > 1e-3)).all(), "hairline contact"
    assert ((iou > 0) == (other > 0)).all(), "the sign of an IoU depends on the angle convention"
    return torch.from_numpy(iou)


ref_loader.box_iou_rotated = box_iou_rotated


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def grid(a, steps=64):
    return (np.round(np.asarray(a, dtype=np.float64) * steps) / steps).astype(np.float32)


def scene(seed: int):
    """A synthetic 8 x 64 sweep (as ``make_golden.py`` ``gen_loader_train_item``), on a grid that is exact in fp32."""
    rng = np.random.default_rng(seed)
    inc = np.linspace(0.2, -0.4, H)[:, None]
    az = np.linspace(math.pi, -math.pi, W)[None, :]
    keep = rng.random((H, W)) >= 0.1
    r = grid(20.0 + 15.0 * np.sin(3 * az) + 10.0 * np.cos(7 * inc) + rng.random((H, W))) * keep
    cols = {"x": grid(r * np.cos(inc) * np.cos(az)), "y": grid(r * np.cos(inc) * np.sin(az)), "z": grid(r * np.sin(inc) * np.ones_like(az)),
            "range": r.astype(np.float32), "intensity": (np.floor(rng.random((H, W)) * 255.0) * keep).astype(np.float32)}
    return {k: v.reshape(-1).astype(np.float32) for k, v in cols.items()}


def quat(yaw):
    yaw = np.asarray(yaw, dtype=np.float64)
    return np.cos(yaw / 2), np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2)


#           name category           tx     ty    l     w    yaw   rows    cols     base range
OBJECTS = (("A", "REGULAR_VEHICLE", 10.5, 0.25, 4.0, 2.0, 0.25, (4, 6), (32, 35), 12.0),
           ("B", "BUS", 30.0, 30.0, 10.0, 3.0, 0.0, (0, 3), (0, 4), 40.0),
           ("C", "BUS", 33.0, 31.0, 10.0, 3.0, 0.5, (1, 4), (2, 6), 44.0),
           ("Z", "BUS", 70.0, 70.0, 10.0, 3.0, 0.0, None, None, 0.0),  # num_interior_pts == 0: filtered by _load_db
           ("D", "PEDESTRIAN", -30.0, -10.0, 1.0, 1.0, 1.0, (2, 5), (10, 14), 10.0),
           ("E", "REGULAR_VEHICLE", -40.0, -20.0, 4.5, 2.0, -0.75, (3, 6), (12, 17), 20.0),
           ("G", "REGULAR_VEHICLE", -50.0, -30.0, 4.5, 2.0, 0.5, (3, 5), (12, 15), 30.0),
           ("K", "BOLLARD", 40.0, -40.0, 0.5, 0.5, 0.0, (0, 2), (40, 42), 55.0),
           ("P", "PEDESTRIAN", 5.0, -30.0, 0.75, 0.75, 2.0, (6, 8), (50, 53), 30.0),
           ("Q", "BUS", -5.0, 45.0, 11.0, 3.0, 2.0, (1, 4), (30, 37), 45.0),
           ("R", "BOLLARD", 45.0, -45.0, 0.5, 0.5, 0.0, (5, 6), (60, 62), 60.0),
           ("T", "REGULAR_VEHICLE", 60.0, 10.0, 4.0, 0.0, 0.0, (6, 8), (5, 7), 60.0),  # degenerate: width 0
           ("U", "PEDESTRIAN", 20.0, -50.0, 0.75, 0.75, -1.0, (5, 7), (20, 22), 50.0))
ROW = {o[0]: i for i, o in enumerate(OBJECTS)}


def write_database(root: Path):
    """``root/db/db.feather`` and ``root/db/train/<category>/<row_nr>.feather``; returns the arrays the tests rebuild it from."""
    rng = np.random.default_rng(77)
    inc = np.linspace(0.2, -0.4, H)
    az = np.linspace(math.pi, -math.pi, W)
    out, npts = {}, []
    for row_nr, (name, cat, tx, ty, ln, wd, yaw, rows, cols, base) in enumerate(OBJECTS):
        if rows is None:
            npts.append(0)
            continue
        rr, cc = np.meshgrid(np.arange(*rows), np.arange(*cols), indexing="ij")
        rr, cc = rr.reshape(-1), cc.reshape(-1)
        r = grid(base + 4.0 * rng.random(rr.size))
        x, y, z = grid(r * np.cos(inc[rr]) * np.cos(az[cc])), grid(r * np.cos(inc[rr]) * np.sin(az[cc])), grid(r * np.sin(inc[rr]))
        inten = np.floor(1.0 + rng.random(rr.size) * 254.0).astype(np.float32)
        if name == "D":  # a point at the origin: it has the smallest range, takes its pixel, and the mask is False there
            r[0], x[0], y[0], z[0] = 0.0, 0.0, 0.0, 0.0
        order = rng.permutation(rr.size)  # the files are not sorted by index
        t = {"index": (rr * W + cc).astype(np.int64)[order], "range": r[order], "x": x[order], "y": y[order], "z": z[order], "intensity": inten[order]}
        path = root / "db" / "train" / cat
        path.mkdir(parents=True, exist_ok=True)
        feather.write_feather(pa.table(t), str(path / f"{row_nr}.feather"), compression="uncompressed")
        npts.append(rr.size)
        for k, v in t.items():
            out[f"db/obj/{row_nr}/{k}"] = v
    qw, qx, qy, qz = quat([o[6] for o in OBJECTS])
    frame = {"timestamp_ns": np.full(len(OBJECTS), 7, dtype=np.int64), "num_interior_pts": np.asarray(npts, dtype=np.int64),
             "category": np.array([o[1] for o in OBJECTS]), "tx_m": np.array([o[2] for o in OBJECTS]), "ty_m": np.array([o[3] for o in OBJECTS]),
             "tz_m": np.linspace(-1.0, 0.5, len(OBJECTS)), "length_m": np.array([o[4] for o in OBJECTS]), "width_m": np.array([o[5] for o in OBJECTS]),
             "height_m": np.full(len(OBJECTS), 1.75), "qw": qw, "qx": qx, "qy": qy, "qz": qz,
             "log_id": np.array([f"log{i % 3}" for i in range(len(OBJECTS))]), "row_nr": np.arange(len(OBJECTS), dtype=np.int64)}
    feather.write_feather(pa.table(frame), str(root / "db" / "db.feather"), compression="uncompressed")
    for k, v in frame.items():
        out[f"db/frame/{k}"] = v
    return out


def scene_annotations():
    yaw = np.array([0.0, 1.0, -0.5, 0.25])
    qw, qx, qy, qz = quat(yaw)
    return {"timestamp_ns": np.array([7, 7, 7, 7], dtype=np.int64), "num_interior_pts": np.array([5, 3, 2, 4], dtype=np.int64),
            "category": np.array(["REGULAR_VEHICLE", "BUS", "PEDESTRIAN", "BUS"]), "tx_m": np.array([10.0, -15.0, 0.0, 25.0]),
            "ty_m": np.array([0.0, 5.0, 20.0, -20.0]), "tz_m": np.array([0.25, 0.5, -0.25, 0.0]), "length_m": np.array([4.5, 11.0, 0.75, 10.0]),
            "width_m": np.array([2.0, 3.0, 0.75, 3.0]), "height_m": np.array([1.5, 3.25, 1.75, 3.0]), "qw": qw, "qx": qx, "qy": qy, "qz": qz}


def tasks_config():
    return DictConfig({"tasks": DictConfig({k: ListConfig(v) for k, v in TASKS.items()})})


def positions(db, category, names):
    part = db[category]._data["row_nr"].tolist()
    return [part.index(ROW[n]) for n in names]


def joined(me, annotations):
    a = annotations.join(me.tasks_frame, on="category").sort(["task_id", "offset"]).collect()  # loader.py:699-704
    return {k: np.asarray(a[k]) for k in a.columns}


def gen_paste(root: Path, out: dict) -> None:
    me = types.SimpleNamespace(root_dir=str(root / "train"), targets_config=tasks_config())
    ref_loader.DataLoader._load_db(me)
    me.tasks_frame = ref_loader.DataLoader.tasks_frame.func(me)
    db = me.db
    assert all("Z" != OBJECTS[r][0] for part in db.values() for r in part._data["row_nr"].tolist())
    cases = {
        "mixed": (True, {"REGULAR_VEHICLE": 3, "BUS": 5, "PEDESTRIAN": 2, "BOLLARD": 1},
                  {"REGULAR_VEHICLE": ["G", "A", "E"], "BUS": ["C", "Q", "B"], "PEDESTRIAN": ["D", "P"], "BOLLARD": ["K"]}),
        "none": (True, {"REGULAR_VEHICLE": 1, "BUS": 2}, {"REGULAR_VEHICLE": ["A"], "BUS": ["B", "C"]}),
        "no_annotations": (False, {"PEDESTRIAN": 3, "REGULAR_VEHICLE": 2}, {"PEDESTRIAN": ["U", "D", "P"], "REGULAR_VEHICLE": ["T", "E"]}),
    }
    for seed, (tag, (with_ann, cfg, picks)) in enumerate(cases.items()):
        table = scene(60 + seed)
        ann = scene_annotations()
        if not with_ann:
            ann = {k: v[:0] for k, v in ann.items()}
        to_img = lambda cols, c: torch.from_numpy(np.stack([table[n] for n in cols]).reshape(c, H, W).copy())  # noqa: E731
        feats, cart = to_img(NAMES, len(NAMES)), to_img(["x", "y", "z"], 3)
        mask = to_img(["range"], 1) > 0
        for k, v in table.items():
            out[f"{tag}/table/{k}"] = v
        for k, v in ann.items():
            out[f"{tag}/ann_in/{k}"] = v
        RECORDED[:] = [positions(db, c, picks[c]) for c in cfg]
        LAST_DRAWS.clear()
        annotations, f2, c2, m2 = ref_loader.sample_database(
            root_dir=root / "db" / "train", database=db, database_config=DictConfig(cfg), annotations=pl.DataFrame(ann), range_view=feats.clone(),
            cart=cart.clone(), range_mask=mask.clone(), lidar_column_names=tuple(NAMES))
        assert not RECORDED
        a = joined(me, annotations)
        out[f"{tag}/db_config/category"], out[f"{tag}/db_config/num_samples"] = np.array(list(cfg)), np.array(list(cfg.values()), dtype=np.int64)
        out[f"{tag}/draws_row_nr"] = np.array([r for d in LAST_DRAWS for r in d], dtype=np.int64)
        out[f"{tag}/features"], out[f"{tag}/cart"], out[f"{tag}/mask"] = f2, c2, m2
        for k, v in a.items():
            out[f"{tag}/ann_out/{k}"] = v
        pasted = int((c2 != cart).any(dim=0).sum())
        print(tag, "draws", LAST_DRAWS, "annotations", len(ann["category"]), "->", a["category"].tolist(), "pixels rewritten", pasted)
        n_in = len(ann["category"])
        if tag == "mixed":
            got = sorted(a["category"].tolist())
            assert len(got) == n_in + 4 and "BOLLARD" not in got  # Q, D, E, P join; A, B, C, G do not; K is pasted without a row
            d0 = out[f"db/obj/{ROW['D']}/index"][out[f"db/obj/{ROW['D']}/range"] == 0][0]
            assert bool(mask.view(-1)[d0]) and not bool(m2.view(-1)[d0]) and float(f2.reshape(len(NAMES), -1)[:, d0].abs().max()) == 0.0
            k0 = int(out[f"db/obj/{ROW['K']}/index"][0])
            assert float(c2.reshape(3, -1)[0, k0]) == float(out[f"db/obj/{ROW['K']}/x"][0])
        elif tag == "none":
            assert len(a["category"]) == n_in and pasted == 0 and torch.equal(f2, feats * mask)
        else:
            assert sorted(a["category"].tolist()) == ["PEDESTRIAN"] * 3 + ["REGULAR_VEHICLE"]


def chain_me(root, table_path, ann_path, aug, enable_db, db_cfg):
    me = types.SimpleNamespace(
        metadata=pl.DataFrame({"log_id": np.array(["log0"]), "timestamp_ns": np.array([7], dtype=np.int64)}), root_dir=str(root / "train"),
        categories=[c for v in TASKS.values() for c in v], annotations_path=lambda log_id: ann_path, lidar_path=lambda log_id, ts: table_path,
        range_view_config=DictConfig({"feature_column_names": NAMES, "filter_roi": False, "height": H, "width": W}), split_name="train",
        augmentations_config=DictConfig({k: DictConfig(v) for k, v in aug.items()}), dataset_name="av2", enable_database=enable_db,
        db_config=DictConfig(db_cfg) if db_cfg else None, x_stride=1, padding_mode="circular", targets_config=tasks_config())
    me.apply_augmentations = types.MethodType(ref_loader.DataLoader.apply_augmentations, me)
    me._point_dropout = types.MethodType(ref_loader.DataLoader._point_dropout, me)
    me.tasks_frame = ref_loader.DataLoader.tasks_frame.func(me)
    if enable_db:
        ref_loader.DataLoader._load_db(me)
    return me


ROT = {"low": -0.78539816, "high": 0.78539816, "p": 1.0}
SCALE = {"low": 0.95, "high": 1.05}
TRANS = {"std_x": 0.5, "std_y": 0.5, "std_z": 0.2}
CHAINS = {
    "second": {"flip_azimuth": {"p": 1.0}, "point_dropout": {"p": 0.8}, "random_rotation": ROT, "random_global_scale": SCALE, "random_global_translation": TRANS},
    "last": {"random_rotation": ROT, "random_global_translation": TRANS, "random_global_scale": SCALE, "flip_azimuth": {"p": 1.0}, "point_dropout": {"p": 0.7}},
    "t_then_s": {"flip_azimuth": {"p": 1.0}, "point_dropout": {"p": 0.75}, "random_global_translation": TRANS, "random_global_scale": SCALE},
}


def gen_chain(root: Path, out: dict) -> None:
    tmp = Path(tempfile.mkdtemp())
    ann = scene_annotations()
    ann_path = tmp / "annotations.feather"
    feather.write_feather(pa.table(ann), str(ann_path), compression="uncompressed")
    for i, (tag, aug) in enumerate(CHAINS.items()):
        table = scene(80 + i)
        me = chain_me(root, None, ann_path, aug, False, None)
        seed = 30 + i
        random.seed(seed)
        np.random.seed(seed)
        sweep, a = me.apply_augmentations(sweep_pl=pl.DataFrame(table), annotations=pl.DataFrame(ann))
        for k, v in table.items():
            out[f"{tag}/table/{k}"] = v
        for k, v in ann.items():
            out[f"{tag}/ann_in/{k}"] = v
        out[f"{tag}/seed"], out[f"{tag}/augmentation_order"] = np.array(seed), np.array(list(aug))
        for k in table:
            out[f"{tag}/out/{k}"] = np.asarray(sweep[k].values if isinstance(sweep[k], _PlSeries) else sweep[k])
        for k in BOX:
            out[f"{tag}/ann_out/{k}"] = np.asarray(a[k].values)
        dropped = (out[f"{tag}/out/intensity"] == 0) & (np.abs(out[f"{tag}/out/x"]) + np.abs(out[f"{tag}/out/y"]) > 0)
        rng_pos = float((out[f"{tag}/out/range"][dropped] > 0).mean()) if dropped.any() else 0.0
        print(tag, "valid", float((out[f"{tag}/out/range"] > 0).mean()), "empty pixels with xyz != 0:", int(dropped.sum()), "of them range > 0:", rng_pos)
        if tag == "t_then_s":
            assert dropped.sum() > 50 and rng_pos == 1.0
    # e2e: __getitem__ with the database, a chain with a mid-chain dropout, and the padding
    table = scene(90)
    table_path = tmp / "sweep.feather"
    feather.write_feather(pa.table(table), str(table_path), compression="uncompressed")
    ann7 = dict(ann, timestamp_ns=np.array([7, 7, 8, 7], dtype=np.int64))
    feather.write_feather(pa.table(ann7), str(ann_path), compression="uncompressed")
    cfg = {"PEDESTRIAN": 2, "BOLLARD": 1, "BUS": 2, "REGULAR_VEHICLE": 2}
    me = chain_me(root, table_path, ann_path, CHAINS["second"], True, cfg)
    seed = 41
    random.seed(seed)
    np.random.seed(seed)
    RECORDED[:] = []
    LAST_DRAWS.clear()
    datum = ref_loader.DataLoader.__getitem__(me, 0)
    a = datum["annotations"]
    for k, v in table.items():
        out[f"e2e/table/{k}"] = v
    for k, v in ann7.items():
        out[f"e2e/ann_in/{k}"] = v
    out["e2e/seed"], out["e2e/augmentation_order"] = np.array(seed), np.array(list(CHAINS["second"]))
    out["e2e/db_config/category"], out["e2e/db_config/num_samples"] = np.array(list(cfg)), np.array(list(cfg.values()), dtype=np.int64)
    out["e2e/draws_row_nr"] = np.array([r for d in LAST_DRAWS for r in d], dtype=np.int64)
    out["e2e/features"], out["e2e/cart"], out["e2e/mask"] = datum["features"], datum["cart"], datum["mask"]
    for k in a.columns:
        out[f"e2e/ann_out/{k}"] = np.asarray(a[k].values)
    print("e2e draws", LAST_DRAWS, "annotations", a["category"].values.tolist(), "features", tuple(datum["features"].shape))
    assert a.shape[0] > 3, "no pasted object survived: pick another seed"


if __name__ == "__main__":
    torch.set_num_threads(1)
    os.makedirs(OUT_DIR, exist_ok=True)
    root = Path(tempfile.mkdtemp())
    (root / "train").mkdir()
    paste = write_database(root)
    gen_paste(root, paste)
    chain: dict = {}
    gen_chain(root, chain)
    for name, arrays in (("paste", paste), ("chain", chain)):
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, **{k: npy(v) for k, v in arrays.items()})
        print(f"database/{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")
