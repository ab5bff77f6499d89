"""Fixtures for ``nms_mode: HARD``: ``tests/golden/nms_hard/{wrapper,decode}.npz``.

Runs the REFERENCE's own ``hard_multiclass_nms`` (``math/ops/nms.py:10-61``), ``batched_multiclass_nms(nms_mode="HARD")``
(``:181-266``) and ``RangeDecoder.decode(use_nms=True)`` (``nn/decoders/range_decoder.py:100-124``) on the CPU.
``detectron2.layers.nms.nms_rotated`` (absent here) is bound to a stand-in with detectron2's signature -- unsorted boxes
``(cx, cy, w, h, angle in degrees)``, scores, ``iou_threshold`` -> kept indices in descending score order -- running the declared
semantics (``include/rv3d.h``) over ``oracle.nms.pairwise_iou``, exactly as ``make_golden.py`` binds ``wnms_gpu``: everything
around the call (class loop, both ``topk`` cuts, ``-yaw.rad2deg()``, float categories, empty shapes) is the reference's.

``wrapper.npz``:

* ``a``  3 sweeps x 2000 candidates x 5 classes in clusters: an absent class, a class with half of the candidates, a sweep with
         nothing >= ``min_confidence``, exact score ties (between boxes that do not overlap: which of two tied boxes is visited
         first is torch's ``topk`` order, which nothing defines); ``num_post_nms`` 1000 / 40 and ``num_pre_nms`` 150;
* ``c``  a hand-built sweep: class 0 holds a suppression chain A > B > C in score at sorted positions 63 / 64 / 65 (IoU(A,B) and
         IoU(B,C) above the threshold, IoU(A,C) below): B is suppressed by A and suppresses nothing, C is kept;
``decode.npz``:

* ``b``  ``decode`` on the tiny model's eval outputs and on the decode fixture (band-sampled and dense): ``(N,10)`` params.

The stand-in asserts on every list it is given that no pair's IoU lies within 1e-4 of the threshold and that boxes with equal
scores do not overlap, and the generator that no ``topk`` cut falls between equal scores -- so no row depends on the unpinned last
bit of the IoU, on the degree -> radian round trip or on a tie rule; the seed of ``a`` is the first one for which this holds.

``wrapper.npz`` is reproducible byte for byte on any CPU, like ``make_golden_assignment.py``'s: its inputs are computed in float64 and
rounded to a grid that is exact in fp32, and every stored row is an input row.  ``decode.npz`` holds scores that went through the
reference's fp32 ``sigmoid``, as ``nms_wrapper.npz`` does: reproducible with the ATen code path the committed file was made with.
"""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stubs and imports the reference)
from make_golden import DictConfig, ListConfig, RangeDecoder, npy  # noqa: E402

from torchbox3d.math.ops import nms as ref_nms  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import nms as onms  # noqa: E402

OUT_DIR = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "nms_hard")
THR, CONF = 0.3, 0.1
MARGIN = 1e-4
FIRST_SEED = 4100


class TooClose(Exception):
    pass


def nms_rotated(boxes, scores, iou_threshold):
    """``detectron2.layers.nms.nms_rotated`` with the declared semantics, on the CPU.  detectron2's ``angle`` runs counter-clockwise in
    image coordinates (y pointing down: the width axis lies at ``(cos a, -sin a)``), so the rectangle's ``ry`` is ``-angle`` in radians --
    with the reference's ``-yaw.rad2deg()`` (nms.py:39) that is the cuboid's own yaw again."""
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and boxes.shape[1] == 5
    thr = float(iou_threshold)
    order = torch.sort(scores, descending=True, stable=True).indices
    b = boxes[order].numpy()
    s = scores[order].numpy()
    half = b[:, 2:4] / np.float32(2)
    rect = np.concatenate([b[:, :2] - half, b[:, :2] + half, (-np.deg2rad(b[:, 4:5].astype(np.float64))).astype(np.float32)], axis=1)
    iou = np.triu(onms.pairwise_iou(rect, rect), 1)
    if iou.size and float(np.abs(iou - np.float32(thr))[np.triu_indices(len(b), 1)].min(initial=1.0)) <= MARGIN:
        raise TooClose("a pair's IoU lies within the margin of the threshold")
    if ((s[:, None] == s[None, :]) & (iou > 0)).any():
        raise TooClose("two overlapping boxes have the same score")
    dead = np.zeros(len(b), dtype=bool)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(i)
        dead |= iou[i] > np.float32(thr)
    return order[torch.as_tensor(keep, dtype=torch.long)]


def cuts_are_clean(sc, cat, pre):
    """No pre-NMS ``topk`` cut falls between two equal scores of a class."""
    for b in range(sc.shape[0]):
        m = sc[b] >= CONF
        for j in cat[b, m].unique():
            s = sc[b, m][cat[b, m] == j].sort(descending=True).values
            if len(s) > pre and float(s[pre - 1]) == float(s[pre]):
                return False
    return True


def grid(t, steps):
    return torch.round(t * steps) / steps


def candidates(g, B, K, n_cls, absent, heavy):
    """(B,K,7) boxes around a few hundred centres plus scattered ones, scores, int64 categories.  float64 draws rounded to a grid."""
    f64 = dict(generator=g, dtype=torch.float64)
    n_ctr = 400
    centres = (torch.rand(B, n_ctr, 2, **f64) - 0.5) * 160.0
    which = torch.randint(0, n_ctr, (B, K), generator=g)
    ctr = torch.gather(centres, 1, which[..., None].expand(B, K, 2))
    scattered = torch.rand(B, K, **f64) > 0.5
    ctr = torch.where(scattered[..., None], (torch.rand(B, K, 2, **f64) - 0.5) * 200.0, ctr + 0.5 * torch.randn(B, K, 2, **f64))
    z = torch.randn(B, K, 1, **f64)
    lwh = torch.tensor([4.5, 2.0, 1.7], dtype=torch.float64) * (1.0 + 0.15 * torch.randn(B, K, 3, **f64)).clamp(0.5, 1.6)
    yaw = (torch.rand(B, K, 1, **f64) * 2 - 1) * math.pi
    yaw_c = torch.gather((torch.rand(B, n_ctr, **f64) * 2 - 1) * math.pi, 1, which)[..., None] + 0.05 * torch.randn(B, K, 1, **f64)
    cub = grid(torch.cat([ctr, z, lwh, torch.where(scattered[..., None], yaw, yaw_c)], dim=-1), 1024).float()
    u = torch.rand(B, K, **f64)
    sc = grid(u * u, 2**20).float()
    cat = torch.randint(0, n_cls, (B, K), generator=g)
    cat = torch.where(torch.rand(B, K, **f64) < 0.5, torch.full_like(cat, heavy), cat)
    cat = torch.where(cat == absent, torch.full_like(cat, (absent + 1) % n_cls), cat)
    return cub, sc, cat


def gen_a(seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    B, K, NCLS = 3, 2000, 5
    cub, sc, cat = candidates(g, B, K, NCLS, absent=3, heavy=1)
    sc[1] = sc[1] * 0.0999  # sweep 1: nothing reaches min_confidence
    sc[2, 0:200:2] = sc[2, 1:200:2]  # sweep 2: exact score ties (the stand-in refuses them between overlapping boxes)
    sc[2, 800:840] = 0.5
    out = {"a/cuboids": cub, "a/scores": sc, "a/categories": cat, "a/seed": np.array(seed)}
    for tag, pre, post in (("post1000", 50000, 1000), ("post40", 50000, 40), ("pre150", 150, 1000)):
        if not cuts_are_clean(sc, cat, pre):
            raise TooClose("a pre-NMS cut between equal scores")
        p, s, c, b = ref_nms.batched_multiclass_nms(cub.clone(), sc.clone(), cat.clone(), num_pre_nms=pre, num_post_nms=post, iou_threshold=THR,
                                                    min_confidence=CONF, nms_mode="hard")
        for i in range(B):
            for j in range(NCLS):
                sj = s[(b == i) & (c == j)]
                if len(sj) == post and tag == "post40":  # the post cut bit: the row behind it must not tie with the last one kept
                    full = ref_nms.batched_multiclass_nms(cub[i:i + 1].clone(), sc[i:i + 1].clone(), cat[i:i + 1].clone(), num_pre_nms=pre,
                                                          num_post_nms=1000, iou_threshold=THR, min_confidence=CONF, nms_mode="HARD")
                    fj = full[1][full[2] == j]
                    if len(fj) > post and float(fj[post]) == float(fj[post - 1]):
                        raise TooClose("a post-NMS cut between equal scores")
        out[f"a/{tag}/params"], out[f"a/{tag}/scores"], out[f"a/{tag}/categories"], out[f"a/{tag}/batch_index"] = p, s, c, b
        out[f"a/{tag}/cfg"] = np.array([pre, post, THR, CONF])
        rows = [[int(((b == i) & (c == j)).sum()) for j in range(NCLS)] for i in range(B)]
        print("a", tag, tuple(p.shape), s.dtype, c.dtype, b.dtype, "rows per sweep and class", rows)
        assert all(r[3] == 0 for r in rows) and sum(rows[1]) == 0 and p.shape[1] == 7
        if tag == "post40":
            assert any(v == 40 for r in rows for v in r)
    n_cand = [(sc[i] >= CONF).sum().item() for i in range(B)]
    heavy = [((sc[i] >= CONF) & (cat[i] == 1)).sum().item() for i in range(B)]
    assert n_cand[1] == 0 and heavy[0] > 0.4 * n_cand[0] and heavy[0] > 150, (n_cand, heavy)
    tied = sc[2][sc[2] >= CONF]
    assert len(tied.unique()) < len(tied) - 60
    # one sweep through hard_multiclass_nms itself
    m = sc[0] >= CONF
    p, s, c = ref_nms.hard_multiclass_nms(cub[0, m], sc[0, m], cat[0, m], iou_threshold=THR, num_pre_nms=50000, num_post_nms=40)
    out["a/multiclass/params"], out["a/multiclass/scores"], out["a/multiclass/categories"] = p, s, c
    # all sweeps empty
    p, s, c, b = ref_nms.batched_multiclass_nms(cub[1:2].clone(), sc[1:2].clone(), cat[1:2].clone(), num_pre_nms=50000, num_post_nms=1000,
                                                iou_threshold=THR, min_confidence=CONF, nms_mode="HARD")
    out["a/empty/params_shape"], out["a/empty/scores_shape"] = np.array(p.shape), np.array(s.shape)
    out["a/empty/categories_shape"], out["a/empty/batch_index_shape"] = np.array(c.shape), np.array(b.shape)
    out["a/empty/categories_is_int64"] = np.array(c.dtype == torch.int64)
    return out


def gen_c() -> dict:
    """Class 0: 63 far-apart boxes with the highest scores, then the chain A, B, C at sorted positions 63, 64, 65, then boxes that
    overlap earlier ones; class 2: a few boxes laid over class 0's (classes do not interact).  Stored in shuffled order."""
    g = torch.Generator().manual_seed(7)
    def box(x, y, yaw):
        return [x, y, 0.25, 4.5, 2.0, 1.75, yaw]
    rows, scores, cats = [], [], []
    for i in range(63):
        rows.append(box(-200.0 + 12.0 * (i % 9), -60.0 + 12.0 * (i // 9), 0.125 * (i % 5)))
        scores.append(0.99 - 0.005 * i)
        cats.append(0)
    for k, x in enumerate((100.0, 101.5, 103.0)):  # A, B, C: IoU(A,B) = IoU(B,C) = 0.5, IoU(A,C) = 0.2
        rows.append(box(x, 40.0, 0.0))
        scores.append(0.5 - 0.01 * k)
        cats.append(0)
    for i in range(30):  # behind the chain: each overlaps one of the first 30 boxes (suppressed) ...
        rows.append(box(-200.0 + 12.0 * (i % 9) + 0.5, -60.0 + 12.0 * (i // 9), 0.125 * (i % 5)))
        scores.append(0.4 - 0.005 * i)
        cats.append(0)
    for i in range(6):  # ... and class 2 over A, B, C and elsewhere
        rows.append(box(100.0 + 0.75 * i, 40.0, 0.0))
        scores.append(0.9 - 0.1 * i)
        cats.append(2)
    perm = torch.randperm(len(rows), generator=g)
    cub = torch.tensor(rows, dtype=torch.float32)[perm][None]
    sc = torch.tensor(scores, dtype=torch.float32)[perm][None]
    cat = torch.tensor(cats, dtype=torch.int64)[perm][None]
    p, s, c, b = ref_nms.batched_multiclass_nms(cub.clone(), sc.clone(), cat.clone(), num_pre_nms=50000, num_post_nms=1000, iou_threshold=THR,
                                                min_confidence=CONF, nms_mode="HARD")
    a_, b_, c_ = (torch.tensor(rows[63 + k], dtype=torch.float32) for k in range(3))
    has = lambda r: bool(((p == r).all(dim=1) & (c == 0)).any())  # noqa: E731
    assert has(a_) and not has(b_) and has(c_), "the chain: A kept, B suppressed, C kept"
    s0 = sc[0][cat[0] == 0].sort(descending=True).values
    assert [float(v) for v in s0[63:66]] == [float(torch.tensor(v, dtype=torch.float32)) for v in (0.5, 0.49, 0.48)]
    assert int((c == 0).sum()) == 65 and int((c == 2).sum()) == 2
    return {"c/cuboids": cub, "c/scores": sc, "c/categories": cat, "c/params": p, "c/scores_out": s, "c/categories_out": c, "c/batch_index": b,
            "c/chain": torch.stack([a_, b_, c_])}


def gen_b() -> dict:
    out: dict = {}
    tm = np.load(make_golden._fixture("tiny_model"))
    dg = np.load(make_golden._fixture("decode"))
    cases = (("tiny", tm["eval/logits"], tm["eval/regressands"], tm["cart"], tm["mask"], True, 1000),
             ("sampled", dg["logits"], dg["regressands"], dg["cart"], dg["mask"], True, 1000),
             ("dense", dg["logits"], dg["regressands"], dg["cart"], dg["mask"], False, 25))
    for tag, logits, reg, cart, mask, sample, postn in cases:
        mo = {1: {"cart": torch.as_tensor(cart), "mask": torch.as_tensor(mask), 0: {"logits": torch.as_tensor(logits), "regressands": torch.as_tensor(reg)}}}
        tasks = DictConfig({0: ListConfig(["c"] * logits.shape[1])})
        dec = RangeDecoder(True, sample, ListConfig([0, 15, 30]), ListConfig([15, 30, math.inf]), ListConfig([8, 2, 1]))
        cfg = DictConfig(num_pre_nms=50000, num_post_nms=postn, nms_threshold=THR, min_confidence=CONF, nms_mode="HARD")
        p, s, c, b = dec.decode(mo, cfg, tasks, use_nms=True)
        assert p.shape[1] == 10 and p.shape[0] > 50
        out[f"b/{tag}/params"], out[f"b/{tag}/scores"], out[f"b/{tag}/categories"], out[f"b/{tag}/batch_index"] = p, s, c, b
        out[f"b/{tag}/num_post_nms"] = np.array(postn)
        print("b", tag, tuple(p.shape), "rows per class", [int((c == j).sum()) for j in range(logits.shape[1])])
    return out


def main() -> None:
    ref_nms.nms_rotated = nms_rotated
    out: dict = {}
    seed = FIRST_SEED
    while True:
        try:
            out.update(gen_a(seed))
            break
        except TooClose as e:
            print(f"seed {seed}: {e}")
            seed += 1
            assert seed < FIRST_SEED + 200
    out.update(gen_c())
    os.makedirs(OUT_DIR, exist_ok=True)
    for name, arrays in (("wrapper", out), ("decode", gen_b())):
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, **{k: npy(v) for k, v in arrays.items()})
        print(f"nms_hard/{name}.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
