"""Object-database sampling ("GT paste") of ``torchbox3d/prototype/loader.py``: ``model.enable_database`` with a ``db_config``
(``conf/dataset/av2.yaml:26-28`` -> ``DataLoader._load_db``, ``loader.py:290-294`` -> ``__getitem__``, ``:672-682`` ->
``sample_database``, ``:708-789``).  Objects cropped from other sweeps are written into the range image, their boxes join the
annotations.  The reference does this per sweep on a DataLoader worker (polars frames, one feather file read per sampled object and
item); here the whole database sits in HBM as one CSR block and a batch is pasted by a fixed number of launches
(``csrc/dbsample.hip``), with ONE small device-to-host copy (which samples survived) for the host-side annotation rows."""

from __future__ import annotations

import os
import random as _random
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from ..engine import _require_cuda

BOX_COLUMNS = ("tx_m", "ty_m", "tz_m", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz")
CART_COLUMNS = ("x", "y", "z")


def _read_feather(path) -> Dict[str, np.ndarray]:
    import pyarrow as pa

    with pa.memory_map(str(path), "r") as src:
        t = pa.ipc.open_file(src).read_all()
    return {name: t.column(name).to_numpy(zero_copy_only=False) for name in t.column_names}


def _write_feather(path, columns: Mapping[str, Any]) -> None:
    import pyarrow as pa

    t = pa.table({k: pa.array(v) for k, v in columns.items()})
    with pa.OSFile(str(path), "wb") as sink, pa.ipc.new_file(sink, t.schema) as writer:  # Feather V2 = the Arrow IPC file format, uncompressed
        writer.write_table(t)


class ObjectDatabase:
    """The reference's object database (``db/db.feather`` + ``db/train/<category>/<row_nr>.feather``) in memory.

    ``boxes`` (N, 10) fp64 in ``BOX_COLUMNS`` order, ``category`` / ``row_nr`` per object, ``by_category``: category -> object ids in
    file order (``partition_by("category")``, ``loader.py:294``); the points of all objects as one CSR block: ``points`` (P, 3 + F)
    fp32 = x, y, z and the columns of ``feature_column_names``, ``range`` (P) fp32, ``index`` (P) int32, ``offsets`` (N + 1) int64.
    :meth:`to` uploads the block once."""

    def __init__(self, boxes, category: Sequence[str], row_nr: Sequence[int], points, range_, index, offsets, feature_column_names: Sequence[str],
                 height: int, width: int, source: str = "<memory>", files: Optional[Sequence[str]] = None) -> None:
        self.boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 10))
        self.category = [str(c) for c in category]
        self.row_nr = [int(r) for r in row_nr]
        self.feature_column_names = list(feature_column_names)
        self.height, self.width = int(height), int(width)
        n, f = len(self.category), len(self.feature_column_names)
        self.points = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3 + f))
        self.range = np.ascontiguousarray(np.asarray(range_, dtype=np.float32).reshape(-1))
        self.index = np.ascontiguousarray(np.asarray(index).reshape(-1)).astype(np.int64)
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        p = self.points.shape[0]
        if self.boxes.shape[0] != n or len(self.row_nr) != n or self.offsets.shape != (n + 1,) or self.range.shape != (p,) or self.index.shape != (p,):
            raise L.RvError(f"object database {source}: {n} objects, {self.boxes.shape[0]} boxes, {self.offsets.shape[0]} offsets, {p} points, "
                            f"{self.range.shape[0]} ranges, {self.index.shape[0]} indices do not fit together")
        if n and (self.offsets[0] != 0 or self.offsets[-1] != p or (np.diff(self.offsets) < 0).any()):
            raise L.RvError(f"object database {source}: the offsets are not a CSR of the {p} points")
        # a bad file on disk must never become an out-of-range store on the device: every index is checked HERE, on the host
        hw = self.height * self.width
        bad = np.nonzero((self.index < 0) | (self.index >= hw))[0]
        if bad.size:
            obj = int(np.searchsorted(self.offsets, bad[0], side="right") - 1)
            name = files[obj] if files is not None else f"object {obj}"
            raise L.RvError(f"object database {name}: pixel index {int(self.index[bad[0]])} outside 0 <= index < height * width = "
                            f"{self.height} * {self.width} = {hw}")
        if p and not (self.range >= 0).all():
            raise L.RvError(f"object database {source}: negative or NaN range (the nearest point is chosen by the bit pattern of range >= 0)")
        self.index = self.index.astype(np.int32)
        self.index_max = int(self.index.max()) if p else -1
        ids: Dict[str, List[int]] = {}
        for i, c in enumerate(self.category):
            ids.setdefault(c, []).append(i)
        self.by_category: Dict[str, np.ndarray] = {c: np.asarray(v, dtype=np.int64) for c, v in ids.items()}
        self.device: Optional[torch.device] = None
        self.d_points = self.d_range = self.d_index = self.d_offsets = None

    def __len__(self) -> int:
        return len(self.category)

    @classmethod
    def from_directory(cls, db_dir, feature_column_names: Sequence[str], height: int, width: int) -> "ObjectDatabase":
        """``_load_db`` (``loader.py:290-294``: ``db.feather`` filtered to ``num_interior_pts > 0``, partitioned by ``category``, rows in file
        order) plus every object's point file (``loader.py:735-739``), read with pyarrow as :func:`..loader.read_sweep_table` does."""
        db_dir = str(db_dir)
        frame = _read_feather(os.path.join(db_dir, "db.feather"))
        rows = np.nonzero(np.asarray(frame["num_interior_pts"]) > 0)[0]
        names = list(feature_column_names)
        boxes = np.stack([np.asarray(frame[c], dtype=np.float64)[rows] for c in BOX_COLUMNS], axis=1) if rows.size else np.zeros((0, 10))
        category = [str(frame["category"][i]) for i in rows]
        row_nr = [int(frame["row_nr"][i]) for i in rows]
        pts, rng, idx, offsets, files = [], [], [], [0], []
        for c, r in zip(category, row_nr):
            path = os.path.join(db_dir, "train", c, f"{r}.feather")
            t = _read_feather(path)
            missing = [n for n in ["index", "range", *CART_COLUMNS, *names] if n not in t]
            if missing:
                raise L.RvError(f"object database {path}: missing columns {missing}")
            pts.append(np.stack([np.asarray(t[n]).astype(np.float32) for n in [*CART_COLUMNS, *names]], axis=1))
            rng.append(np.asarray(t["range"]).astype(np.float32))
            idx.append(np.asarray(t["index"]).astype(np.int64))
            offsets.append(offsets[-1] + len(idx[-1]))
            files.append(path)
        f = len(names)
        return cls(boxes, category, row_nr, np.concatenate(pts) if pts else np.zeros((0, 3 + f), np.float32),
                   np.concatenate(rng) if rng else np.zeros(0, np.float32), np.concatenate(idx) if idx else np.zeros(0, np.int64),
                   np.asarray(offsets, dtype=np.int64), names, height, width, source=db_dir, files=files)

    def to(self, device="cuda") -> "ObjectDatabase":
        """Upload the CSR block (once; the paste reads it from HBM)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.RvError("ObjectDatabase.to needs a CUDA (ROCm) device: the hot path has no CPU fallback")
        self.d_points = torch.from_numpy(self.points).to(dev)
        self.d_range = torch.from_numpy(self.range).to(dev)
        self.d_index = torch.from_numpy(self.index).to(dev)
        self.d_offsets = torch.from_numpy(self.offsets).to(dev)
        self.device = self.d_points.device
        return self


def draw_database_samples(db: ObjectDatabase, db_config: Mapping[str, int], rng=_random) -> List[int]:
    """Step 1 of ``sample_database`` (``loader.py:718-727``) for ONE sweep: for each ``(category, num_samples)`` of ``db_config``, in
    config order, ``min(rows of the category, num_samples)`` DISTINCT objects of that category, concatenated -> object ids of ``db``.

    The reference draws with polars' own generator (``DataFrame.sample``), which nothing outside polars can reproduce; this function
    draws with ``rng.sample`` (Python's ``random`` by default).  Only the DISTRIBUTION is the same -- a uniform draw without replacement
    per category -- not the stream: a seeded run does not pick the objects a seeded reference run picks.  The draw is its own function so
    that recorded draws (tests; users who want polars' stream) can be handed to :func:`paste_database` instead.  A category of
    ``db_config`` that the database does not hold is a ``KeyError``, as ``database[k]`` is in the reference."""
    out: List[int] = []
    for category, num_samples in db_config.items():
        ids = db.by_category[str(category)]
        n = min(len(ids), int(num_samples))
        if n > 0:
            out.extend(int(i) for i in rng.sample([int(i) for i in ids], n))
    return out


def _yaw(rows: np.ndarray) -> np.ndarray:
    w, x, y, z = rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9]
    return np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))  # euler_from_quaternion's yaw (utils/polars.py:18)


def bev_rectangles(rows: np.ndarray) -> np.ndarray:
    """(n, >= 10) fp64 rows in ``COLS`` order -> (n, 5) fp32 ``[x1, y1, x2, y2, ry]`` of ``rv_rotated_iou`` (``csrc/nms_geom.h``).
    The reference hands ``[tx, ty, length, width, yaw]`` in fp32 to mmcv's ``box_iou_rotated`` (``loader.py:775-788``), whose box has
    its first extent along ``(cos a, sin a)``: the rectangle with the length axis at +yaw."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(-1, rows.shape[-1])
    b = np.stack([rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4], _yaw(rows)], axis=1).astype(np.float32)
    half = np.float32(0.5)
    return np.stack([b[:, 0] - half * b[:, 2], b[:, 1] - half * b[:, 3], b[:, 0] + half * b[:, 2], b[:, 1] + half * b[:, 3], b[:, 4]], axis=1)


def task_frame(tasks: Mapping[Any, Sequence[str]]) -> Dict[str, Any]:
    """``tasks_frame`` (``loader.py:553-565``): category -> (task_id, offset in the SORTED category list of the task)."""
    frame = {}
    for k, cats in tasks.items():
        for offset, c in enumerate(sorted(cats)):
            frame[str(c)] = (int(k), offset)
    return frame


def merge_annotations(annotations: Optional[Tensor], db: ObjectDatabase, survivors: Sequence[Sequence[int]], tasks: Mapping[Any, Sequence[str]]) -> Tensor:
    """Step 7: ``concat([annotations, surviving samples])`` (``loader.py:774``), then the inner join with the task frame and the stable
    sort by ``(task_id, offset)`` at the end of ``__getitem__`` (``:699-704``), sweep by sweep.  Pasted rows of a category outside
    ``tasks`` vanish in the join; among equal keys the scene's rows come first, then pasted rows in sample order.  (M, 13) fp64 rows in
    ``COLS`` order; ``survivors[b]``: object ids of sweep b in sample order."""
    frame = task_frame(tasks)
    ann = torch.zeros((0, 13), dtype=torch.float64) if annotations is None else torch.as_tensor(annotations).double().reshape(-1, 13)
    parts = []
    for b, ids in enumerate(survivors):
        scene = ann[ann[:, 12] == b]
        ids = [i for i in ids if db.category[i] in frame]
        pasted = torch.zeros((len(ids), 13), dtype=torch.float64)
        for r, i in enumerate(ids):
            pasted[r, :10] = torch.from_numpy(db.boxes[i])
            pasted[r, 10], pasted[r, 11], pasted[r, 12] = frame[db.category[i]][0], frame[db.category[i]][1], b
        rows = torch.cat([scene, pasted])
        order = sorted(range(rows.shape[0]), key=lambda j: (float(rows[j, 10]), float(rows[j, 11])))  # stable, as polars' sort
        parts.append(rows[order])
    rest = ann[(ann[:, 12] < 0) | (ann[:, 12] >= len(survivors))]
    if rest.shape[0]:
        raise L.RvError(f"annotations hold batch_index values outside 0 .. {len(survivors) - 1}")
    return torch.cat(parts) if parts else ann


def paste_database(batch: Mapping[str, Any], db: ObjectDatabase, draws: Sequence[Sequence[int]], tasks: Mapping[Any, Sequence[str]]) -> Dict[str, Any]:
    """Steps 2-7 of ``sample_database`` (``loader.py:728-774``) on an UNPADDED batch dict with :func:`..loader.augment_batch`'s contract
    (``features`` (B, F, H, W) fp32, ``cart`` (B, 3, H, W) fp32, ``mask`` (B, 1, H, W) bool, ``annotations`` (M, 13) fp64 host rows or
    absent); ``draws[b]``: the object ids drawn for sweep b (:func:`draw_database_samples`, or recorded draws).

    Collision (``:728-733``): ``rv_rotated_iou`` of annotations x samples and samples x samples for all sweeps at once, compared to 0 on
    the device -- a sample that touches a scene box goes, then BOTH members of a colliding pair of survivors go (and a degenerate box,
    whose IoU with itself is 0).  Points (``:735-772``): ``rv_db_paste_keys`` / ``rv_db_paste_resolve`` -- the nearest point wins each
    pixel (ties: the earlier sample, then the earlier point), a pasted point always overwrites the scene's pixel, every pixel leaves with
    ``features * mask``.  Samples that own no pixel leave (``:744-745``).  ONE device-to-host copy (B x S bytes: kept and owning) follows
    the launches; the annotation merge is host work on a handful of rows (:func:`merge_annotations`).  Pasted objects are not augmented
    (the reference pastes after the augmentations).  Returns a new dict; ``pasted[b]`` lists the surviving object ids of sweep b."""
    feats, cart, mask = batch["features"], batch["cart"], batch["mask"]
    _require_cuda(feats, "features")
    B, F, H, W = feats.shape
    if W != db.width or H != db.height:
        raise L.RvError(f"paste_database on a batch of height x width {H} x {W}, the database was made for {db.height} x {db.width}: paste BEFORE "
                        "the W padding (range_view_from_table(..., pad=False) -> augment_batch -> paste_database -> pad_batch)")
    if F != len(db.feature_column_names):
        raise L.RvError(f"paste_database: the batch has {F} feature channels, the database {len(db.feature_column_names)} ({db.feature_column_names})")
    if len(draws) != B:
        raise L.RvError(f"paste_database: {len(draws)} draws for a batch of {B} sweeps")
    if db.device is None or db.device != feats.device:
        raise L.RvError(f"paste_database: the database is on {db.device}, the batch on {feats.device} (ObjectDatabase.to(device) uploads it once)")
    out = dict(batch)
    ann = batch.get("annotations")
    ann = torch.zeros((0, 13), dtype=torch.float64) if ann is None else torch.as_tensor(ann).double().reshape(-1, 13)
    S = max([len(d) for d in draws] + [0])
    if S == 0:  # nothing drawn (the reference's ``pl.concat([])`` raises here): the batch passes through
        out["annotations"], out["pasted"] = merge_annotations(ann, db, [[] for _ in range(B)], tasks), [[] for _ in range(B)]
        return out
    samples = np.full((B, S), -1, dtype=np.int32)
    for b, d in enumerate(draws):
        d = np.asarray(list(d), dtype=np.int64)
        if d.size and (d.min() < 0 or d.max() >= len(db)):
            raise L.RvError(f"paste_database: sweep {b} draws object {int(d.max() if d.max() >= len(db) else d.min())}, the database holds {len(db)}")
        samples[b, : d.size] = d
    flat = samples.reshape(-1)
    valid = flat >= 0
    counts = np.diff(db.offsets)
    max_work = int(counts[flat[valid]].sum())
    rect_s = np.zeros((B * S, 5), dtype=np.float32)  # empty slots: degenerate rectangles (IoU 0 with everything)
    rect_s[valid] = bev_rectangles(db.boxes[flat[valid]])
    rect_a = bev_rectangles(ann.numpy()) if ann.shape[0] else np.zeros((0, 5), dtype=np.float32)
    dev = feats.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)  # noqa: E731
    M = int(ann.shape[0])
    with torch.cuda.device(dev):
        rect_s_d, samples_d = up(rect_s), up(flat)
        slot_b = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(S)
        keep = samples_d >= 0
        if M:
            rect_a_d, ann_b = up(rect_a), up(ann[:, 12].numpy().astype(np.int32))
            iou_as = torch.empty((M, B * S), dtype=torch.float32, device=dev)
            L.call("rv_rotated_iou", L.ptr(rect_a_d), M, L.ptr(rect_s_d), B * S, L.ptr(iou_as), L.stream_ptr())
            keep = keep & ~((iou_as > 0) & (ann_b[:, None] == slot_b[None, :])).any(dim=0)  # loader.py:728-731
        iou_ss = torch.empty((B * S, B * S), dtype=torch.float32, device=dev)
        L.call("rv_rotated_iou", L.ptr(rect_s_d), B * S, L.ptr(rect_s_d), B * S, L.ptr(iou_ss), L.stream_ptr())
        hits = ((iou_ss > 0) & (slot_b[:, None] == slot_b[None, :]) & keep[:, None]).sum(dim=0)
        keep = (keep & (hits == 1)).to(torch.uint8).contiguous()  # loader.py:732-733: exactly one hit, the sample itself
        owned = torch.empty(B * S, dtype=torch.uint8, device=dev)
        ws = torch.empty(int(L.load().rv_db_paste_workspace_bytes(B, S, H, W)), dtype=torch.uint8, device=dev)
        f_in, c_in, m_in = feats.float().contiguous(), cart.float().contiguous(), mask.to(torch.uint8).contiguous()
        f_out, c_out, m_out = torch.empty_like(f_in), torch.empty_like(c_in), torch.empty_like(m_in)
        L.call("rv_db_paste_keys", L.ptr(samples_d), L.ptr(keep), B, S, L.ptr(db.d_offsets), len(db), L.ptr(db.d_range),
               L.ptr(db.d_index), db.index_max, max_work, H, W, L.ptr(owned), L.ptr(ws), L.stream_ptr())
        L.call("rv_db_paste_resolve", L.ptr(f_in), L.ptr(c_in), L.ptr(m_in), L.ptr(f_out), L.ptr(c_out), L.ptr(m_out), B, F, H,
               W, L.ptr(samples_d), S, L.ptr(db.d_offsets), L.ptr(db.d_points), L.ptr(ws), L.ptr(owned), L.stream_ptr())
        alive = (keep & owned).cpu().numpy().reshape(B, S)  # the ONE device-to-host copy, after everything is enqueued
    out["features"], out["cart"], out["mask"] = f_out, c_out, m_out.bool()
    out["pasted"] = [[int(samples[b, s]) for s in range(S) if alive[b, s]] for b in range(B)]
    out["annotations"] = merge_annotations(ann, db, out["pasted"], tasks)
    return out


def extract_interior_pixels(cart: Tensor, mask: Tensor, annotations: Tensor):
    """``rv_db_extract``: for every annotation row (``COLS`` order, ``batch_index`` last, grouped by sweep) the flat pixel indices of its
    sweep with ``mask`` true that lie inside the cuboid (the interior test of the target assignment, ``math/polytope.py:14-56``),
    ascending.  Returns (offsets (m + 1) int64, index (n) int32) on the host."""
    _require_cuda(cart, "cart")
    B, _, H, W = cart.shape
    ann = torch.as_tensor(annotations).double().reshape(-1, 13)
    m = int(ann.shape[0])
    if m == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    bi = ann[:, 12].numpy().astype(np.int64)
    if (np.diff(bi) < 0).any() or bi.min() < 0 or bi.max() >= B:
        raise L.RvError("extract_interior_pixels: annotation rows must be grouped by sweep (batch_index ascending, 0 .. B - 1)")
    cub = np.zeros((m, 10), dtype=np.float64)
    cub[:, :6], cub[:, 6], cub[:, 9] = ann[:, :6].numpy(), _yaw(ann.numpy()), bi
    dev = cart.device
    offs = np.concatenate([[0], np.cumsum(np.bincount(bi, minlength=B))]).astype(np.int32)
    with torch.cuda.device(dev):
        cub_d, offs_d = torch.from_numpy(cub).to(dev), torch.from_numpy(offs).to(dev)
        c32, m8 = cart.float().contiguous(), mask.to(torch.uint8).contiguous()
        counts = torch.empty(m, dtype=torch.int64, device=dev)
        obj_offsets = torch.empty(m + 1, dtype=torch.int64, device=dev)
        args = (L.ptr(c32), L.ptr(m8), B, H, W, L.ptr(cub_d), m, L.ptr(offs_d), L.ptr(counts), L.ptr(obj_offsets))
        L.call("rv_db_extract", *args, L.ptr(None), 0, L.stream_ptr())
        host_offsets = obj_offsets.cpu().numpy()
        total = int(host_offsets[-1])
        index = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        if total:
            L.call("rv_db_extract", *args, L.ptr(index), total, L.stream_ptr())
        return host_offsets, index[:total].cpu().numpy()


def build_object_database(tables: Sequence[Mapping[str, Any]], annotations: Sequence[Mapping[str, Any]], range_view_config: Mapping[str, Any],
                          dataset_name: str, dst_dir, device="cuda") -> int:
    """Write an object database in the layout ``sample_database`` reads: ``dst_dir/db.feather`` (the annotation columns ``BOX_COLUMNS``
    plus ``category``, ``num_interior_pts``, ``log_id``, ``row_nr``) and one ``dst_dir/train/<category>/<row_nr>.feather`` per object with
    at least one point (``index`` = flat pixel of the unpadded image, ``range``, ``x``, ``y``, ``z`` and the feature columns as the image
    holds them).  The reference ships NO builder -- its database was made outside the repository -- so there is nothing to match beyond
    what its reader expects (``loader.py:290-294, 735-762``).

    ``tables[i]``: the sweep table of :func:`..loader.range_view_from_table`; ``annotations[i]``: that sweep's annotation columns
    (``BOX_COLUMNS``, ``category`` and optionally ``log_id``).  An object's points are the valid pixels inside its cuboid
    (``rv_db_extract``); a pixel inside two overlapping cuboids belongs to both.  Returns the number of objects written."""
    from .loader import range_view_from_table

    names = list(range_view_config["feature_column_names"])
    items = [range_view_from_table(t, range_view_config, dataset_name, device=device, pad=False) for t in tables]
    feats, cart, mask = (torch.stack([it[k] for it in items]) for k in ("features", "cart", "mask"))
    rows, cats, logs = [], [], []
    for b, a in enumerate(annotations):
        n = len(a["category"])
        r = np.zeros((n, 13), dtype=np.float64)
        for j, c in enumerate(BOX_COLUMNS):
            r[:, j] = np.asarray(a[c], dtype=np.float64)
        r[:, 12] = b
        rows.append(r)
        cats += [str(c) for c in np.asarray(a["category"]).tolist()]
        logs += [str(v) for v in np.asarray(a["log_id"]).tolist()] if "log_id" in a else [""] * n
    ann = np.concatenate(rows) if rows else np.zeros((0, 13))
    offsets, index = extract_interior_pixels(cart, mask, torch.from_numpy(ann))
    hw = feats.shape[-2] * feats.shape[-1]
    idx_d = torch.from_numpy(index.astype(np.int64)).to(feats.device)
    sweep_of = np.repeat(ann[:, 12].astype(np.int64), np.diff(offsets)) if len(cats) else np.zeros(0, dtype=np.int64)
    flat_d = torch.from_numpy(sweep_of).to(feats.device) * hw + idx_d
    gather = lambda x: x.permute(1, 0, 2, 3).reshape(x.shape[1], -1)[:, flat_d].cpu().numpy()  # noqa: E731  (C, n)
    f_h, c_h = gather(feats), gather(cart)
    rng_h = np.stack([np.asarray(t["range"]).astype(np.float32) for t in tables]).reshape(-1)[sweep_of * hw + index] if len(index) else np.zeros(0, np.float32)
    dst_dir = str(dst_dir)
    os.makedirs(os.path.join(dst_dir, "train"), exist_ok=True)
    for k, c in enumerate(cats):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        if hi == lo:
            continue
        os.makedirs(os.path.join(dst_dir, "train", c), exist_ok=True)
        cols: Dict[str, Any] = {"index": index[lo:hi].astype(np.int64), "range": rng_h[lo:hi]}
        for j, n in enumerate(CART_COLUMNS):
            cols[n] = c_h[j, lo:hi]
        for j, n in enumerate(names):
            if n not in cols:
                cols[n] = f_h[j, lo:hi]
        _write_feather(os.path.join(dst_dir, "train", c, f"{k}.feather"), cols)
    frame: Dict[str, Any] = {c: ann[:, j] for j, c in enumerate(BOX_COLUMNS)}
    frame.update(category=cats, num_interior_pts=np.diff(offsets).astype(np.int64), log_id=logs, row_nr=np.arange(len(cats), dtype=np.int64))
    _write_feather(os.path.join(dst_dir, "db.feather"), frame)
    return len(cats)
