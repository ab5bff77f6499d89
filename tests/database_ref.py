"""numpy restatement of the reference's ``sample_database`` (``prototype/loader.py:708-789``) plus the join and sort at the end of
``__getitem__`` (``:699-704``), for ONE sweep -- the yardstick of tests/test_gpu_database.py where no fixture exists, itself checked against
``tests/golden/database/paste.npz`` (tests/test_database_golden.py).  Ties in range go to the earlier (sample, point) position: the
declared rule of ``rv_db_paste_keys`` (the reference leaves them to an unstable sort)."""

from __future__ import annotations

import os

import numpy as np

from oracle import nms as onms

BOX = ("tx_m", "ty_m", "tz_m", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz")


def rectangles(rows):
    """(n, >= 10) fp64 [tx ty tz l w h qw qx qy qz ...] -> (n, 5) fp32 [x1, y1, x2, y2, ry] with ry = +yaw (``loader.py:775-788``)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1])
    w, x, y, z = rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 9]
    yaw = np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
    b = np.stack([rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4], yaw], axis=1).astype(np.float32)
    h = np.float32(0.5)
    return np.stack([b[:, 0] - h * b[:, 2], b[:, 1] - h * b[:, 3], b[:, 0] + h * b[:, 2], b[:, 1] + h * b[:, 3], b[:, 4]], axis=1)


def iou(a, b):
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), dtype=np.float32)
    return onms.pairwise_iou(a, b)


def paste_sweep(features, cart, mask, ann, boxes, category, points, rng, index, offsets, draws, tasks, batch_index=0):
    """features (F,H,W) fp32, cart (3,H,W), mask (1,H,W) bool, ann (M,13) fp64 rows of this sweep; the database as host arrays (``boxes``
    (N,10), ``category``, CSR ``points`` (P,3+F) / ``rng`` / ``index`` / ``offsets``); ``draws``: object ids in sample order.
    Returns features, cart, mask, annotations (M',13), the surviving object ids."""
    features, cart, mask = features.copy(), cart.copy(), mask.copy()
    draws = [int(d) for d in draws]
    rs = rectangles(boxes[draws]) if draws else np.zeros((0, 5), np.float32)
    keep = (iou(rectangles(ann), rs) > 0).sum(axis=0) == 0 if len(ann) else np.ones(len(draws), dtype=bool)
    alive = [d for d, k in zip(draws, keep) if k]
    rs = rs[keep]
    keep = (iou(rs, rs) > 0).sum(axis=0) == 1 if alive else np.zeros(0, dtype=bool)
    alive = [d for d, k in zip(alive, keep) if k]
    F = features.shape[0]
    f, c, m = features.reshape(F, -1), cart.reshape(3, -1), mask.reshape(1, -1)
    owners = set()
    if alive:
        pts = np.concatenate([np.arange(offsets[d], offsets[d + 1]) for d in alive])
        owner = np.concatenate([np.full(offsets[d + 1] - offsets[d], d) for d in alive])
        order = np.argsort(rng[pts], kind="stable")
        pts, owner = pts[order], owner[order]
        _, first = np.unique(index[pts], return_index=True)
        pts, owner = pts[first], owner[first]
        owners = set(owner.tolist())
        px = index[pts]
        f[:, px] = points[pts, 3:].T
        c[:, px] = points[pts, :3].T
        m[:, px] = np.linalg.norm(points[pts, :3], axis=-1) > 0.0
    f *= m
    alive = [d for d in alive if d in owners]
    frame = {str(cat): (int(k), o) for k, cats in tasks.items() for o, cat in enumerate(sorted(cats))}
    rows = [np.asarray(r, dtype=np.float64) for r in ann]
    for d in alive:
        if category[d] in frame:
            rows.append(np.concatenate([boxes[d], [frame[category[d]][0], frame[category[d]][1], batch_index]]))
    rows.sort(key=lambda r: (r[10], r[11]))
    out = np.stack(rows) if rows else np.zeros((0, 13))
    return features, cart, mask, out, alive


def write_db_dir(g, root) -> str:
    """The database of ``paste.npz`` (``db/frame/*``, ``db/obj/<row_nr>/*``) as a directory in the reference's layout."""
    import pyarrow as pa

    def write(path, cols):
        t = pa.table({k: pa.array(v) for k, v in cols.items()})
        with pa.OSFile(str(path), "wb") as sink, pa.ipc.new_file(sink, t.schema) as w:
            w.write_table(t)

    root = str(root)
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    frame = {k[len("db/frame/"):]: g.np(k) for k in g.keys if k.startswith("db/frame/")}
    write(os.path.join(root, "db.feather"), frame)
    for row_nr, cat in zip(frame["row_nr"].tolist(), frame["category"].tolist()):
        cols = {k.rsplit("/", 1)[1]: g.np(k) for k in g.keys if k.startswith(f"db/obj/{row_nr}/")}
        if cols:
            os.makedirs(os.path.join(root, "train", str(cat)), exist_ok=True)
            write(os.path.join(root, "train", str(cat), f"{row_nr}.feather"), cols)
    return root


def case_inputs(g, tag, names, H, W):
    """Unpadded images and the (M,13) annotation rows of a fixture case (the filter / join / sort of ``annotations_for_sweep``)."""
    table = {k[len(f"{tag}/table/"):]: g.np(k) for k in g.keys if k.startswith(f"{tag}/table/")}
    ann_in = {k[len(f"{tag}/ann_in/"):]: g.np(k) for k in g.keys if k.startswith(f"{tag}/ann_in/")}
    feats = np.stack([table[n] for n in names]).reshape(len(names), H, W)
    cart = np.stack([table[n] for n in ("x", "y", "z")]).reshape(3, H, W)
    return table, ann_in, feats, cart, (table["range"] > 0).reshape(1, H, W)


def ann_out_rows(g, tag):
    cols = [g.np(f"{tag}/ann_out/{c}").astype(np.float64) for c in BOX + ("task_id", "offset")]
    return np.stack(cols, axis=1) if len(cols[0]) else np.zeros((0, 12))
