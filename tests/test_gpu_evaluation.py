"""Detection evaluation on the device (``rv_eval_match`` / ``rv_eval_summarize``, ``evaluation.DetectionEvaluator`` / ``evaluate``)
against the hand-computed cases of ``tests/golden/eval_cases.json`` and the NumPy restatement of the declared semantics
(``tests/eval_ref.py``).

Bar: flags, ``evaluated`` and ``matched_gt`` are decided on fp64 squares of fp32 inputs and are EXACT; the error columns are fp64
results rounded to fp32 (1e-5); the summary fed the device's own flags agrees with ``np.interp`` to 1e-9, end to end to 1e-6; the
table is bit-identical from run to run and under any split of the same rows into ``update`` calls.
"""

from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch

import eval_ref as ref
from test_evaluation_cpu import CASES, _cfg, check_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _run(scene, cfg):
    """Scene arrays (as ``eval_ref.load_cases`` lays them out) through ``match`` and ``summarize``; numpy results."""
    from range_view_3d_detection_amd.evaluation import match, summarize

    n_cat, n_seg = scene["n_cat"], scene["n_sweeps"] * scene["n_cat"]
    dt_cat, gt_cat = _dev(scene["dt_cat"]), _dev(scene["gt_cat"])
    out = match(_dev(scene["dts"]), _dev(scene["scores"]), _dev(scene["dt_sweep"]) * n_cat + dt_cat, _dev(scene["gts"]),
                _dev(scene["gt_valid"]), _dev(scene["gt_sweep"]) * n_cat + gt_cat, n_seg, cfg)
    n_gt = torch.zeros(n_cat, dtype=torch.int64, device=DEV).index_add_(0, gt_cat, out["gt_evaluated"].long())
    table, ap_t, n_dts = summarize(_dev(scene["scores"]), dt_cat, out["evaluated"], out["tp"], out["err"], n_gt, cfg)
    return {k: v.cpu().numpy() for k, v in out.items()}, n_gt.cpu().numpy(), table.numpy(), ap_t.numpy(), n_dts.numpy()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_computed_cases(case):
    out, n_gt, table, _, n_dts = _run(case, _cfg(case["n_cat"]))
    check_case(case, out, table)
    assert n_dts.sum() == np.sum(case["expect"]["evaluated"]) and n_gt.sum() == np.sum(case["expect"]["gt_evaluated"])


def _scene(g, n_sweeps, n_cat, max_gt=60, max_dt=1000, big=None):
    """Random sweeps: per (sweep, category) 0 .. max_gt ground truths and 0 .. max_dt detections drawn around them (sigma 0.3 .. 3 m),
    scores on a coarse grid (ties), some rows beyond 150 m, some categories empty on either side, rows in shuffled order.
    ``big`` = (sweep, category, ground truths[, detections = 400]): one segment with that many boxes."""
    dts, scores, dt_s, dt_c, gts, npts, gt_s, gt_c = [], [], [], [], [], [], [], []
    for s in range(n_sweeps):
        for c in range(n_cat):
            m = int(g.integers(0, max_gt + 1)) if g.random() > 0.15 else 0
            n = int(g.integers(0, max_dt + 1) if g.random() < 0.2 else g.integers(0, 150)) if g.random() > 0.15 else 0
            if big and (s, c) == big[:2]:
                m, n = big[2], big[3] if len(big) > 3 else 400
            centre = np.concatenate([g.uniform(-160, 160, (m, 2)), g.uniform(-2, 2, (m, 1))], 1)
            gt = np.concatenate([centre, g.uniform(0.5, 6, (m, 3)), g.uniform(-math.pi, math.pi, (m, 1))], 1)
            gts.append(gt), npts.append(g.integers(0, 4, m)), gt_s.append(np.full(m, s)), gt_c.append(np.full(m, c))
            if m:
                src = gt[g.integers(0, m, n)]
                dt = src + np.concatenate([g.normal(0, 1, (n, 3)) * g.uniform(0.3, 3, (n, 1)), g.normal(0, 0.3, (n, 3)), g.normal(0, 0.5, (n, 1))], 1)
                dt[:, 3:6] = np.abs(dt[:, 3:6]) + 0.1
            else:
                dt = np.concatenate([g.uniform(-160, 160, (n, 2)), g.uniform(-2, 2, (n, 1)), g.uniform(0.5, 6, (n, 3)), g.uniform(-3, 3, (n, 1))], 1)
            dts.append(dt), scores.append(np.round(g.random(n), 2)), dt_s.append(np.full(n, s)), dt_c.append(np.full(n, c))
    dts, gts = np.concatenate(dts), np.concatenate(gts)
    pd, pg = g.permutation(len(dts)), g.permutation(len(gts))
    return {"n_sweeps": n_sweeps, "n_cat": n_cat, "dts": ref.rows_from_yaw(dts)[pd], "scores": np.concatenate(scores).astype(np.float32)[pd],
            "dt_sweep": np.concatenate(dt_s).astype(np.int64)[pd], "dt_cat": np.concatenate(dt_c).astype(np.int64)[pd],
            "gts": ref.rows_from_yaw(gts)[pg], "gt_valid": (np.concatenate(npts) > 0).astype(np.uint8)[pg],
            "gt_sweep": np.concatenate(gt_s).astype(np.int64)[pg], "gt_cat": np.concatenate(gt_c).astype(np.int64)[pg]}


def _against_restatement(scene, cfg):
    out, n_gt, table, ap_t, n_dts = _run(scene, cfg)
    want, want_n_gt, want_table, want_ap_t = ref.evaluate_ref(scene["dts"], scene["scores"], scene["dt_sweep"], scene["dt_cat"], scene["gts"],
                                                              scene["gt_valid"], scene["gt_sweep"], scene["gt_cat"], scene["n_sweeps"], scene["n_cat"], cfg)
    for key in ("evaluated", "tp", "matched_gt", "gt_evaluated"):
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(np.isnan(out["err"]), np.isnan(want["err"]))
    assert np.allclose(out["err"], want["err"], rtol=0, atol=1e-5, equal_nan=True)
    assert np.array_equal(n_gt, want_n_gt)
    assert np.array_equal(n_dts, [np.sum((scene["dt_cat"] == c) & (want["evaluated"] != 0)) for c in range(scene["n_cat"])])
    # the summary alone, fed the device's flags and fp32 errors: only the order of the fp64 sums differs
    fed_table, fed_ap_t = ref.summarize_ref(scene["scores"], scene["dt_cat"], out["evaluated"], out["tp"], out["err"], n_gt, scene["n_cat"], cfg)
    assert np.allclose(ap_t, fed_ap_t, rtol=1e-9, atol=1e-12) and np.allclose(table, fed_table, rtol=1e-9, atol=1e-12)
    assert np.allclose(table, want_table, rtol=0, atol=1e-6) and np.allclose(ap_t, want_ap_t, rtol=0, atol=1e-6)
    return out, table


def test_random_scenes_against_the_restatement():
    g = np.random.default_rng(np.random.randint(1 << 30))  # (seeded from this test's name: tests/conftest.py)
    scene = _scene(g, 8, 26)
    seg_sizes = np.bincount(scene["dt_sweep"] * 26 + scene["dt_cat"], minlength=8 * 26)
    assert seg_sizes.max() > 400 and (seg_sizes == 0).sum() > 10 and len(scene["gts"]) > 3000
    out, table = _against_restatement(scene, _cfg(26))
    assert (out["evaluated"] == 0).sum() > 1000 and out["tp"][:, 2].sum() > 300 and 0.01 < table[-1, 0] < 0.95
    assert (np.linalg.norm(scene["dts"][:, :3], axis=1) > 150).sum() > 100


def test_a_segment_with_more_ground_truth_than_one_lds_chunk():
    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _scene(g, 2, 3, max_gt=20, max_dt=200, big=(1, 2, 3000))
    out, _ = _against_restatement(scene, _cfg(3, max_num_dts_per_category=300))
    in_big = (scene["dt_sweep"] == 1) & (scene["dt_cat"] == 2)
    big_gt_rows = np.nonzero((scene["gt_sweep"] == 1) & (scene["gt_cat"] == 2))[0]
    matched = out["matched_gt"][in_big & (out["matched_gt"] >= 0)]
    # matches land in the second and third chunk of the segment too
    assert len(matched) > 100 and (np.searchsorted(big_gt_rows, matched) >= 2048).sum() > 10


def _evaluator_table(scene, cfg, splits, names):
    from range_view_3d_detection_amd.evaluation import DetectionEvaluator

    ev = DetectionEvaluator(cfg, names, max_sweeps=scene["n_sweeps"])
    ann = np.zeros((len(scene["gts"]), 13))
    ann[:, :10], ann[:, 11], ann[:, 12] = scene["gts"], scene["gt_cat"], scene["gt_sweep"]
    for sweeps in np.array_split(np.arange(scene["n_sweeps"]), splits):
        d, a = np.isin(scene["dt_sweep"], sweeps), np.isin(scene["gt_sweep"], sweeps)
        ev.update(_dev(scene["dts"][d]), _dev(scene["scores"][d]), _dev(scene["dt_cat"][d], torch.float32), _dev(scene["dt_sweep"][d], torch.float32),
                  _dev(ann[a]), num_interior_pts=_dev(scene["gt_valid"][a]))
    return ev.compute()


def test_order_independence_and_repeatability():
    """One ``update`` or four (accumulation order of equal keys kept), run twice: the same table bit for bit; and equal to the
    functional path on the whole scene."""
    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _scene(g, 8, 5, max_gt=40, max_dt=400)
    # rows grouped by sweep (stable), so that splitting by sweep keeps the accumulation order of ties
    by_sweep = np.argsort(scene["dt_sweep"], kind="stable")
    for k in ("dts", "scores", "dt_sweep", "dt_cat"):
        scene[k] = scene[k][by_sweep]
    cfg, names = _cfg(5), [f"C{i}" for i in range(5)]
    tables = [_evaluator_table(scene, cfg, splits, names) for splits in (1, 4, 1, 4, 8)]
    for t in tables[1:]:
        assert t.equals(tables[0])
    _, n_gt, table, _, n_dts = _run(scene, cfg)
    assert tables[0].column("category").to_pylist() == names + ["AVERAGE_METRICS"]
    for j, name in enumerate(("AP", "ATE", "ASE", "AOE", "CDS")):
        assert np.array_equal(np.asarray(tables[0].column(name)), table[:, j]), name
    assert tables[0].column("n_dts").to_pylist() == n_dts.tolist() + [n_dts.sum()] and tables[0].column("n_gts").to_pylist() == n_gt.tolist() + [n_gt.sum()]


def test_update_does_not_synchronise_and_counts_stray_rows():
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.evaluation import DetectionEvaluator

    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _scene(g, 4, 3, max_gt=20, max_dt=200)
    ann = np.zeros((len(scene["gts"]), 13))
    ann[:, :10], ann[:, 11], ann[:, 12] = scene["gts"], scene["gt_cat"], scene["gt_sweep"]
    args = (_dev(scene["dts"]), _dev(scene["scores"]), _dev(scene["dt_cat"], torch.float32), _dev(scene["dt_sweep"], torch.float32), _dev(ann))
    ev = DetectionEvaluator(_cfg(3), ["C0", "C1", "C2"], max_sweeps=4)
    ev.update(*args)  # (first call: library load, lookup tables)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):  # grows the accumulators on the way
            ev.update(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    table = ev.compute()
    assert table.num_rows == 4 and 0 < table.column("AP")[3].as_py() < 1
    ev.reset()
    ev.update(*args, n_sweeps=2)  # sweeps 2 and 3 fall outside the grid: counted on the device, reported by compute()
    with pytest.raises(RvError, match="batch_index outside"):
        ev.compute()


def test_decoder_output_through_update_equals_the_offline_form(golden, tmp_path):
    """``RangeDecoder.decode`` of the tiny model's eval outputs + annotations -> ``update`` -> ``compute`` equals ``evaluate()`` on the
    Arrow tables ``write_detections`` wrote, read back; two tasks, so annotation rows carry (task_id, offset)."""
    import pyarrow as pa

    from range_view_3d_detection_amd.evaluation import DetectionEvaluator, detection_cfg_factory, evaluate
    from range_view_3d_detection_amd.math.ops.coding import DETECTION_COLUMNS, build_dataframe, write_detections
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

    t = golden("tiny_model")
    logits, reg, cart, mask = t["eval/logits"], t["eval/regressands"], t["cart"], t["mask"]
    n_cls, B = logits.shape[1], logits.shape[0]
    assert n_cls >= 2
    tasks = {0: [f"K{i}" for i in range(n_cls - 1)], 1: ["Z"]}
    names = tasks[0] + tasks[1]
    mo = {1: {"cart": cart.to(DEV), "mask": mask.to(DEV), 0: {"logits": logits[:, :n_cls - 1].to(DEV), "regressands": reg.to(DEV)},
              1: {"logits": logits[:, n_cls - 1:].to(DEV), "regressands": reg.to(DEV)}}}
    post = {"num_pre_nms": 50000, "num_post_nms": 200, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "HARD"}
    params, scores, cats, bidx = RangeDecoder(True, False, [], [], []).decode(mo, post, tasks, use_nms=True)
    assert params.shape[0] > 20 and cats.dtype.is_floating_point
    # ground truth: every third detection, moved by up to ~1.5 m; annotation rows as the loader lays them out
    g = torch.Generator().manual_seed(7)
    pick = torch.arange(0, params.shape[0], 3)
    box = params[pick].double().cpu()
    box[:, :3] += torch.randn(len(pick), 3, generator=g, dtype=torch.float64) * 0.8
    cls = cats[pick].long().cpu()
    ann = torch.cat([box, (cls == n_cls - 1).double()[:, None], torch.where(cls == n_cls - 1, 0, cls).double()[:, None], bidx[pick].double().cpu()[:, None]], 1)
    cfg = detection_cfg_factory("av2", names)
    ev = DetectionEvaluator(cfg, names, tasks=tasks)
    ev.update(params, scores, cats, bidx, ann, n_sweeps=B)
    online = ev.compute()
    uuids = {"batch_index": list(range(B)), "log_id": [f"log{b // 2}" for b in range(B)], "timestamp_ns": [1000 + b for b in range(B)]}
    paths = write_detections(build_dataframe(params, scores, cats, bidx, uuids, names), str(tmp_path), "run")
    dts = pa.concat_tables([pa.ipc.open_file(p).read_all() for p in paths])
    b = ann[:, 12].long().tolist()
    gts = pa.table({**{c: pa.array(ann[:, j].float().numpy()) for j, c in enumerate(DETECTION_COLUMNS)},
                    "category": [names[int(k)] for k in cls], "num_interior_pts": [5] * len(b),
                    "log_id": [uuids["log_id"][i] for i in b], "timestamp_ns": [uuids["timestamp_ns"][i] for i in b]})
    dts_out, gts_out, offline = evaluate(dts, gts, cfg, device=DEV)
    assert offline.equals(online)
    assert online.column("category").to_pylist() == sorted(names) + ["AVERAGE_METRICS"]
    assert online.column("AP")[-1].as_py() > 0.05 and sum(online.column("n_gts").to_pylist()[:-1]) == len(b)
    assert dts_out.num_rows == dts.num_rows and {"is_evaluated", "tp_0.5", "tp_4.0", "ATE", "ASE", "AOE"} <= set(dts_out.column_names)
    assert all(gts_out.column("is_evaluated").to_pylist())
    tp2 = np.asarray(dts_out.column("tp_2.0").to_pylist())
    assert tp2.sum() > 5 and np.array_equal(~np.isnan(np.asarray(dts_out.column("ATE").to_pylist(), dtype=np.float64)), tp2)


def test_compute_gathers_over_the_process_group(tmp_path):
    """With ``torch.distributed`` initialised ``compute()`` goes through the gather (sizes, padded rows, summed counts): on a
    one-rank group it must return the table of the plain path."""
    import torch.distributed as dist

    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _scene(g, 2, 3, max_gt=20, max_dt=100)
    cfg, names = _cfg(3), ["C0", "C1", "C2"]
    plain = _evaluator_table(scene, cfg, 1, names)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    try:
        assert _evaluator_table(scene, cfg, 1, names).equals(plain)
    finally:
        dist.destroy_process_group()
