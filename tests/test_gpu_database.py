"""Object-database paste (``rv_db_paste_keys`` / ``rv_db_paste_resolve``), the builder (``rv_db_extract``) and the mid-chain
``point_dropout`` (``rv_augment_dropout``) on the device, against the fixtures of ``tests/golden/database/`` (the reference's own
``sample_database`` / ``apply_augmentations`` / ``__getitem__``) and, where no fixture exists, the numpy restatement ``tests/database_ref.py``.
Bar: ``features`` / ``cart`` / ``mask`` of a paste EXACTLY (every value is a copy or a product with 0 / 1), annotations equal; the
augmentation chain as tests/test_gpu_loader_train.py (1e-6 of the channel maximum, mask exact)."""

from __future__ import annotations

import random

import numpy as np
import pytest
import torch

import database_ref as ref
from test_database_golden import CASES, H, NAMES, TASKS, W, draws_of, load_db, scene_rows
from test_gpu_forward import DEV

pytestmark = pytest.mark.gpu


def batch_of(g, tags, device=DEV):
    feats, carts, masks, anns = [], [], [], []
    for b, tag in enumerate(tags):
        _, ann_in, f, c, m = ref.case_inputs(g, tag, NAMES, H, W)
        rows = scene_rows(ann_in)
        rows[:, 12] = b
        feats.append(f), carts.append(c), masks.append(m), anns.append(rows)
    to = lambda xs: torch.from_numpy(np.stack(xs)).to(device)  # noqa: E731
    return {"features": to(feats), "cart": to(carts), "mask": to(masks), "annotations": torch.from_numpy(np.concatenate(anns))}


def check_case(g, tag, out, b):
    assert out["mask"].dtype == torch.bool
    assert np.array_equal(out["features"][b].cpu().numpy(), g.np(f"{tag}/features")), tag
    assert np.array_equal(out["cart"][b].cpu().numpy(), g.np(f"{tag}/cart")), tag
    assert np.array_equal(out["mask"][b].cpu().numpy(), g.np(f"{tag}/mask")), tag
    rows = out["annotations"].numpy()
    assert np.array_equal(rows[rows[:, 12] == b][:, :12], ref.ann_out_rows(g, tag)), tag


@pytest.mark.parametrize("tags", [(t,) for t in CASES] + [CASES, CASES[::-1]])
def test_fixture_cases_through_paste_database(golden, tmp_path, tags):
    from range_view_3d_detection_amd.prototype.database import paste_database

    g, db = load_db(golden, tmp_path)
    db.to(DEV)
    batch = batch_of(g, tags)
    before = {k: batch[k].clone() for k in ("features", "cart", "mask")}
    out = paste_database(batch, db, [draws_of(g, db, t) for t in tags], TASKS)
    for b, tag in enumerate(tags):
        check_case(g, tag, out, b)
    assert all(torch.equal(batch[k], before[k]) for k in before)  # the input batch is left alone
    assert out["annotations"][:, 12].tolist() == sorted(out["annotations"][:, 12].tolist())


def test_zero_size_paths_and_refusals(golden, tmp_path):
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.prototype.database import paste_database

    g, db = load_db(golden, tmp_path)
    batch = batch_of(g, ("mixed", "no_annotations"))
    with pytest.raises(L.RvError, match="ObjectDatabase.to"):
        paste_database(batch, db, [[0], [1]], TASKS)
    db.to(DEV)
    out = paste_database(batch, db, [[], []], TASKS)  # no samples: the batch passes through
    assert torch.equal(out["features"], batch["features"]) and torch.equal(out["annotations"], batch["annotations"]) and out["pasted"] == [[], []]
    no_ann = {k: v for k, v in batch.items() if k != "annotations"}
    out = paste_database(no_ann, db, [draws_of(g, db, "no_annotations")] * 2, TASKS)  # no annotations at all
    assert np.array_equal(out["cart"][1].cpu().numpy(), g.np("no_annotations/cart")) and out["annotations"].shape == (8, 13)
    out = paste_database(batch, db, [draws_of(g, db, "none"), []], TASKS)  # every sample rejected; an empty slot row
    assert out["pasted"] == [[], []] and torch.equal(out["cart"], batch["cart"]) and torch.equal(out["mask"], batch["mask"])
    assert torch.equal(out["features"], batch["features"] * batch["mask"]) and torch.equal(out["annotations"], batch["annotations"])
    with pytest.raises(L.RvError, match="BEFORE the W padding"):
        paste_database({k: (v[..., :60] if k != "annotations" else v) for k, v in batch.items()}, db, [[0], [1]], TASKS)
    with pytest.raises(L.RvError, match="the database holds 12"):
        paste_database(batch, db, [[12], []], TASKS)


def synthetic_database(n_obj, h, w, seed):
    """Random objects on an h x w image: blocks of pixels, ranges on a coarse grid (so that ties in range occur), boxes scattered in BEV."""
    from range_view_3d_detection_amd.prototype.database import ObjectDatabase

    rng = np.random.default_rng(seed)
    pts, rngs, idx, offsets, boxes, cats = [], [], [], [0], [], []
    for i in range(n_obj):
        hh, ww = int(rng.integers(1, 12)), int(rng.integers(1, 60))
        r0, c0 = int(rng.integers(0, h - hh + 1)), int(rng.integers(0, w - ww + 1))
        rr, cc = np.meshgrid(np.arange(r0, r0 + hh), np.arange(c0, c0 + ww), indexing="ij")
        sel = rng.random(rr.size) < 0.8
        sel[0] = True
        px = (rr.reshape(-1) * w + cc.reshape(-1))[sel]
        n = px.size
        r = (np.round(rng.uniform(5, 60) + rng.random(n) * 4.0) * 0.5).astype(np.float32)  # half-metre grid: many equal ranges
        xyz = (rng.normal(size=(n, 3)) * 20).astype(np.float32)
        xyz[rng.random(n) < 0.02] = 0.0
        pts.append(np.concatenate([xyz, rng.random((n, 1)).astype(np.float32) * 255, r[:, None], xyz], axis=1))
        rngs.append(r), idx.append(px), offsets.append(offsets[-1] + n)
        yaw = rng.uniform(-np.pi, np.pi)
        wd = 0.0 if i % 97 == 0 else rng.uniform(0.5, 3)
        boxes.append([rng.uniform(-100, 100), rng.uniform(-100, 100), 0.0, rng.uniform(0.5, 10), wd, 1.5, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
        cats.append(["REGULAR_VEHICLE", "BUS", "PEDESTRIAN", "BOLLARD"][i % 4])
    return ObjectDatabase(np.asarray(boxes), cats, list(range(n_obj)), np.concatenate(pts), np.concatenate(rngs), np.concatenate(idx), np.asarray(offsets),
                          NAMES, h, w)


def test_full_size_batch_is_exact_and_deterministic():
    """4 x 64 x 1800 with 150 drawn objects per sweep, against the numpy restatement; the same paste twice gives identical bits (the tie
    rule -- equal ranges on one pixel go to the earlier (slot, point) -- does not depend on scheduling)."""
    from bench import synthetic_batch
    from range_view_3d_detection_amd.prototype.database import paste_database

    B, h, w, S = 4, 64, 1800, 150
    db = synthetic_database(1200, h, w, 5).to(DEV)
    sb = synthetic_batch(B, h, w, seed=9, device="cpu", boxes_per_sweep=12, n_cls=3)
    ann = np.zeros((sb["annotations"].shape[0], 13))
    ann[:] = np.asarray(sb["annotations"], dtype=np.float64).reshape(-1, 13)
    ann[:, 10], ann[:, 11] = 0, ann[:, 11] % 2
    order = np.lexsort((ann[:, 11], ann[:, 10], ann[:, 12]))
    ann = ann[order]
    batch = {"features": sb["features"].float().to(DEV), "cart": sb["cart"].to(DEV), "mask": sb["mask"].to(DEV), "annotations": torch.from_numpy(ann)}
    rng = random.Random(2)
    draws = [rng.sample(range(len(db)), S) for _ in range(B)]
    out = paste_database(batch, db, draws, TASKS)
    again = paste_database(batch, db, draws, TASKS)
    for k in ("features", "cart", "mask"):
        assert torch.equal(out[k].view(torch.uint8) if k == "mask" else out[k].view(torch.int32), again[k].view(torch.uint8) if k == "mask" else again[k].view(torch.int32)), k
    assert out["pasted"] == again["pasted"] and sum(len(p) for p in out["pasted"]) > 100
    f, c, m = (batch[k].cpu().numpy() for k in ("features", "cart", "mask"))
    rows = []
    for b in range(B):
        fb, cb, mb, ab, alive = ref.paste_sweep(f[b], c[b], m[b], ann[ann[:, 12] == b], db.boxes, db.category, db.points, db.range, db.index, db.offsets,
                                                draws[b], TASKS, batch_index=b)
        assert alive == out["pasted"][b], b
        assert np.array_equal(out["features"][b].cpu().numpy(), fb) and np.array_equal(out["cart"][b].cpu().numpy(), cb), b
        assert np.array_equal(out["mask"][b].cpu().numpy(), mb), b
        rows.append(ab)
    assert np.array_equal(out["annotations"].numpy(), np.concatenate(rows))


ROT = {"low": -0.78539816, "high": 0.78539816, "p": 1.0}
AUG = {"flip_azimuth": {"p": 1.0}, "random_rotation": ROT, "random_global_scale": {"low": 0.95, "high": 1.05},
       "random_global_translation": {"std_x": 0.5, "std_y": 0.5, "std_z": 0.2}}
DROP_P = {"second": 0.8, "last": 0.7, "t_then_s": 0.75, "e2e": 0.8}


def aug_config(g, tag):
    cfg = dict(AUG, point_dropout={"p": DROP_P[tag]})
    return {k: cfg[k] for k in [str(n) for n in g.np(f"{tag}/augmentation_order")]}


def close(got, want, what):
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-6 * max(1.0, float(np.abs(want).max())), what


@pytest.mark.parametrize("tag", ["second", "last", "t_then_s"])
def test_mid_chain_dropout_through_augment_batch(golden, tag):
    """``point_dropout`` second / last in a chain, and followed by translation then scale (a dropped pixel gets a POSITIVE range and counts
    as valid, as in the reference)."""
    from range_view_3d_detection_amd.prototype import loader as ld

    g = golden("database/chain")
    table = {k[len(f"{tag}/table/"):]: g.np(k) for k in g.keys if k.startswith(f"{tag}/table/")}
    cfg = {"feature_column_names": NAMES, "filter_roi": False, "height": H, "width": W}
    item = ld.range_view_from_table(table, cfg, "av2", device=DEV, pad=False)
    batch = {k: v[None] for k, v in item.items()}
    seed = int(g.np(f"{tag}/seed"))
    random.seed(seed)
    np.random.seed(seed)  # the keep mask comes from numpy's global generator, as in the reference
    out = ld.augment_batch(batch, NAMES, aug_config(g, tag), width=W)
    want = {n: g.np(f"{tag}/out/{n}").reshape(H, W) for n in NAMES}
    assert np.array_equal(out["mask"][0, 0].cpu().numpy(), want["range"] > 0), tag
    got = out["features"][0].cpu().numpy()
    assert np.array_equal(got[0], want["intensity"]), tag  # a placement channel: bit for bit
    for i, n in enumerate(NAMES[1:], 1):
        close(got[i], want[n], (tag, n))
    close(out["cart"][0].cpu().numpy(), np.stack([want[n] for n in ("x", "y", "z")]), tag)
    if tag == "t_then_s":
        empty = want["intensity"] == 0
        assert empty.sum() > 50 and (got[1][empty] > 0).all()


def test_train_batch_with_database_matches_the_reference_chain(golden, tmp_path):
    """``train_batch_from_tables`` with ``db``: table -> image -> augmentations (mid-chain dropout) -> paste -> mask + W padding against the
    reference's ``__getitem__`` with ``enable_database``; the database draw is ``random.sample`` on both sides."""
    from range_view_3d_detection_amd.prototype import loader as ld

    g, db = load_db(golden, tmp_path)
    db.to(DEV)
    c = golden("database/chain")
    tag = "e2e"
    table = {k[len(f"{tag}/table/"):]: c.np(k) for k in c.keys if k.startswith(f"{tag}/table/")}
    ann_in = {k[len(f"{tag}/ann_in/"):]: c.np(k) for k in c.keys if k.startswith(f"{tag}/ann_in/")}
    cfg = {"feature_column_names": NAMES, "filter_roi": False, "height": H, "width": W}
    db_config = {str(k): int(v) for k, v in zip(c.np(f"{tag}/db_config/category"), c.np(f"{tag}/db_config/num_samples"))}
    seed = int(c.np(f"{tag}/seed"))
    random.seed(seed)
    np.random.seed(seed)
    ann = ld.annotations_for_sweep(ann_in, 7, TASKS)
    out = ld.train_batch_from_tables([table], ann, cfg, "av2", aug_config(c, tag), 1, "circular", device=DEV, db=db, db_config=db_config, tasks=TASKS)
    want_rows = [db.row_nr.index(int(r)) for r in c.np(f"{tag}/draws_row_nr")]
    assert set(out["pasted"][0]) <= set(want_rows) and len(out["pasted"][0]) >= 1
    assert np.array_equal(out["mask"][0].cpu().numpy(), c.np(f"{tag}/mask"))
    got, want = out["features"][0].cpu().numpy(), c.np(f"{tag}/features")
    assert np.array_equal(got[0], want[0])
    for i, n in enumerate(NAMES[1:], 1):
        close(got[i], want[i], n)
    close(out["cart"][0].cpu().numpy(), c.np(f"{tag}/cart"), "cart")
    rows = out["annotations"].numpy()
    assert rows[:, 10].tolist() == c.np(f"{tag}/ann_out/task_id").tolist() and rows[:, 11].tolist() == c.np(f"{tag}/ann_out/offset").tolist()
    want_a = np.stack([c.np(f"{tag}/ann_out/{k}") for k in ref.BOX[:6]], axis=1)
    assert np.max(np.abs(rows[:, :6] - want_a)) <= 1e-9 * max(1.0, float(np.abs(want_a).max()))
    # defaults leave the chain as it was
    random.seed(seed)
    np.random.seed(seed)
    a = ld.train_batch_from_tables([table], ann, cfg, "av2", aug_config(c, tag), 1, "circular", device=DEV)
    random.seed(seed)
    np.random.seed(seed)
    b = ld.train_batch_from_tables([table], ann, cfg, "av2", aug_config(c, tag), 1, "circular", device=DEV, db=None, db_config=None, tasks=None)
    assert all(torch.equal(a[k], b[k]) for k in ("features", "cart", "mask", "annotations"))


def synthetic_scene_tables(B, h, w, seed):
    from bench import synthetic_batch

    sb = synthetic_batch(B, h, w, seed=seed, device="cpu", boxes_per_sweep=6, n_cls=3)
    ann = np.asarray(sb["annotations"], dtype=np.float64).reshape(-1, 13)
    tables, anns = [], []
    cats = ["BUS", "PEDESTRIAN", "REGULAR_VEHICLE"]
    for b in range(B):
        cart = sb["cart"][b].numpy().reshape(3, -1)
        valid = sb["mask"][b].numpy().reshape(-1)
        rng_col = (np.linalg.norm(cart, axis=0) * valid).astype(np.float32)
        tables.append({"x": cart[0] * valid, "y": cart[1] * valid, "z": cart[2] * valid, "range": rng_col,
                       "intensity": (np.arange(h * w) % 251).astype(np.float32) * valid})
        rows = ann[ann[:, 12] == b]
        a = {c: rows[:, j] for j, c in enumerate(ref.BOX)}
        a["category"] = np.array([cats[int(o) % 3] for o in rows[:, 11]])
        anns.append(a)
    return tables, anns


def test_builder_round_trip(tmp_path):
    """``build_object_database`` on a synthetic scene, read back, one object pasted into an EMPTY image: exactly its pixels come back."""
    from range_view_3d_detection_amd.prototype.database import ObjectDatabase, build_object_database, paste_database

    h, w = 16, 128
    cfg = {"feature_column_names": NAMES, "filter_roi": False, "height": h, "width": w}
    tables, anns = synthetic_scene_tables(2, h, w, 4)
    n = build_object_database(tables, anns, cfg, "av2", tmp_path / "db", device=DEV)
    assert n == sum(len(a["category"]) for a in anns)
    db = ObjectDatabase.from_directory(tmp_path / "db", NAMES, h, w).to(DEV)
    assert len(db) >= 3
    counts = np.diff(db.offsets)
    obj = int(np.argmax(counts))
    lo, hi = db.offsets[obj], db.offsets[obj + 1]
    assert (np.diff(db.index[lo:hi]) > 0).all()  # ascending index: the fill pass does not depend on scheduling
    sweep = 0 if db.row_nr[obj] < len(anns[0]["category"]) else 1
    # the object's pixels are the valid pixels of its sweep inside its cuboid (host restatement of the slab test, fp64)
    t = tables[sweep]
    bx = db.boxes[obj]
    yaw = 2 * np.arctan2(bx[9], bx[6])
    dx, dy, dz = t["x"] - bx[0], t["y"] - bx[1], t["z"] - bx[2]
    u, v = np.cos(yaw) * dx + np.sin(yaw) * dy, -np.sin(yaw) * dx + np.cos(yaw) * dy
    inside = (np.abs(u) <= bx[3] / 2 - 1e-4) & (np.abs(v) <= bx[4] / 2 - 1e-4) & (np.abs(dz) <= bx[5] / 2 - 1e-4) & (t["range"] > 0)
    assert set(np.nonzero(inside)[0].tolist()) <= set(db.index[lo:hi].tolist())
    loose = (np.abs(u) <= bx[3] / 2 + 1e-4) & (np.abs(v) <= bx[4] / 2 + 1e-4) & (np.abs(dz) <= bx[5] / 2 + 1e-4) & (t["range"] > 0)
    assert set(db.index[lo:hi].tolist()) <= set(np.nonzero(loose)[0].tolist())
    empty = {"features": torch.zeros(1, len(NAMES), h, w, device=DEV), "cart": torch.zeros(1, 3, h, w, device=DEV),
             "mask": torch.zeros(1, 1, h, w, dtype=torch.bool, device=DEV)}
    out = paste_database(empty, db, [[obj]], {0: ["BUS", "PEDESTRIAN", "REGULAR_VEHICLE"]})
    assert out["pasted"] == [[obj]] and out["annotations"].shape == (1, 13)
    got = np.nonzero(out["mask"][0, 0].cpu().numpy().reshape(-1))[0]
    assert np.array_equal(got, db.index[lo:hi])
    f = out["features"][0].cpu().numpy().reshape(len(NAMES), -1)
    for j, name in enumerate(NAMES):
        assert np.array_equal(f[j, got], t[name][got]), name
    assert np.array_equal(out["cart"][0].cpu().numpy().reshape(3, -1)[:, got], np.stack([t[k][got] for k in ("x", "y", "z")]))


def test_training_step_on_a_pasted_batch(tmp_path):
    """The hand-off to the target assignment: one training step of the tiny detector on a pasted batch; the loss is finite and every
    pasted annotation owns at least one target pixel."""
    from bench import Detector, build_model
    from range_view_3d_detection_amd.prototype import loader as ld
    from range_view_3d_detection_amd.prototype.database import ObjectDatabase, build_object_database

    h, w = 16, 120  # 128 columns after the W padding of 4 + 4
    cfg = {"feature_column_names": NAMES, "filter_roi": False, "height": h, "width": w}
    src_tables, src_anns = synthetic_scene_tables(2, h, w, 6)
    build_object_database(src_tables, src_anns, cfg, "av2", tmp_path / "db", device=DEV)
    db = ObjectDatabase.from_directory(tmp_path / "db", NAMES, h, w).to(DEV)
    tasks = {0: ["BUS", "PEDESTRIAN", "REGULAR_VEHICLE"]}
    tables, _ = synthetic_scene_tables(2, h, w, 8)
    torch.manual_seed(0)
    backbone, head = build_model("c32", 3)
    model = Detector(backbone, head).to(DEV).train()
    out = ld.train_batch_from_tables(tables, None, cfg, "av2", None, 1, "constant", rng=random.Random(1), device=DEV, db=db,
                                     db_config={"BUS": 2, "PEDESTRIAN": 2, "REGULAR_VEHICLE": 2}, tasks=tasks)
    n_pasted = sum(len(p) for p in out["pasted"])
    assert n_pasted >= 2 and out["annotations"].shape == (n_pasted, 13) and out["features"].shape[-1] == w + 8
    data = {k: out[k] for k in ("features", "cart", "mask", "annotations")}
    feats = model.backbone(data)
    outputs, losses = model.head(feats, data, return_loss=True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(losses["loss"])
    pan = data[1][0]["panoptics"].cpu()
    for b in range(2):
        assert len(pan[b].unique()) - 1 == len(out["pasted"][b]), (b, pan[b].unique().tolist(), out["pasted"][b])
