"""``nms_mode: HARD`` on the device: ``rv_nms_sweeps_hard`` (device-resident batch path), the reference-shaped per-class loop over
``rv_nms_rotated`` and the detectron2-shaped shim, against the fixtures of ``tests/golden/nms_hard/`` (the reference's own wrapper code)
and, where no fixture exists, against the numpy restatement of the declared semantics (``tests/nms_hard_ref.py``).

Bar: hard NMS is a selection, and the CPU IoU equals the device's bit for bit -- so row order, classes and batch index are exact and
boxes / scores are ``torch.equal`` to the selected INPUT rows.  Both device paths and the restatement break score ties by ascending
candidate index, so against the restatement even tied rows are compared in place; against the fixtures (torch's ``topk`` order inside
the reference) tie groups are canonicalised as tests/test_gpu_nms_wrapper.py does.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import nms_hard_ref as ref
from nms_hard_ref import same_rows_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _both_paths(fn):
    """Run ``fn()`` on the device-resident path and with the per-class loop forced."""
    from range_view_3d_detection_amd.math.ops import nms as hnms

    fast = fn()
    old = hnms.FUSED_CLASSES_MAX
    hnms.FUSED_CLASSES_MAX = 0
    try:
        loop = fn()
    finally:
        hnms.FUSED_CLASSES_MAX = old
    return {"rv_nms_sweeps_hard": fast, "per-class loop": loop}


def _equals_restatement(got, cub, sc, cat, cfg, what):
    """``got`` = the four tensors of ``batched_multiclass_nms``: exactly the rows the restatement selects, in its order."""
    bi, ki, ci = ref.batched(cub, sc, cat, *cfg)
    p, s, c, b = (t.cpu() for t in got)
    assert p.shape[0] == bi.size, (what, p.shape[0], bi.size)
    if bi.size == 0:
        assert tuple(p.shape) == (0, 7) and tuple(s.shape) == (0, 1) and tuple(c.shape) == (0, 1) and tuple(b.shape) == (0, 1), what
        return 0
    assert c.dtype == sc.dtype and b.dtype == sc.dtype and p.dtype == cub.dtype, what
    assert np.array_equal(c.numpy().astype(np.int64), ci), f"{what}: categories / row order differ"
    assert np.array_equal(b.numpy().astype(np.int64), bi), f"{what}: batch index differs"
    bi, ki = torch.from_numpy(bi), torch.from_numpy(ki)
    assert torch.equal(s, sc.cpu()[bi, ki]), f"{what}: scores are not the selected input scores"
    assert torch.equal(p, cub.cpu()[bi, ki]), f"{what}: boxes are not the selected input rows"
    return int(bi.numel())


def _clustered(sizes, seed, n_centres=6, jitter=0.6, spread=60.0, tie_every=0):
    """One sweep: ``sizes[j]`` boxes of class j jittered around a few centres per class (what a range-view head emits: hundreds of
    near-copies of one object), shuffled; scores in (0.05, 1), every ``tie_every``-th one copied from its neighbour."""
    g = torch.Generator().manual_seed(seed)
    cubs, cats = [], []
    for j, n in enumerate(sizes):
        if n == 0:
            continue
        centres = (torch.rand(n_centres, 2, generator=g) - 0.5) * spread
        yaws = (torch.rand(n_centres, 1, generator=g) * 2 - 1) * math.pi
        which = torch.randint(0, n_centres, (n,), generator=g)
        ctr = centres[which] + jitter * torch.randn(n, 2, generator=g)
        lwh = torch.tensor([4.5, 2.0, 1.7]) * (1.0 + 0.1 * torch.randn(n, 3, generator=g)).clamp(0.6, 1.5)
        yaw = yaws[which] + 0.08 * torch.randn(n, 1, generator=g)
        cubs.append(torch.cat([ctr, torch.randn(n, 1, generator=g), lwh, yaw], dim=1))
        cats.append(torch.full((n,), j, dtype=torch.int64))
    cub, cat = torch.cat(cubs).float(), torch.cat(cats)
    sc = (0.05 + 0.95 * torch.rand(cub.shape[0], generator=g)).float()
    if tie_every:
        idx = torch.arange(0, sc.numel() - 1, tie_every)
        sc[idx] = sc[idx + 1]
    perm = torch.randperm(cub.shape[0], generator=g)
    return cub[perm], sc[perm], cat[perm]


def _pad_stack(sweeps):
    """Sweeps of different sizes -> one batch: padding candidates get score 0 (below every ``min_confidence`` used here)."""
    K = max(s[0].shape[0] for s in sweeps)
    cub = torch.zeros(len(sweeps), K, 7)
    sc = torch.zeros(len(sweeps), K)
    cat = torch.zeros(len(sweeps), K, dtype=torch.int64)
    for i, (c, s, k) in enumerate(sweeps):
        cub[i, : c.shape[0]], sc[i, : c.shape[0]], cat[i, : c.shape[0]] = c, s, k
        cub[i, c.shape[0]:, 3:6] = 1.0
    return cub, sc, cat


# ------------------------------------------------------------------------------------------------------------------
# 1. the fixtures
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["post1000", "post40", "pre150"])
def test_batched_multiclass_nms_hard_against_the_reference_wrapper(golden, tag):
    from range_view_3d_detection_amd.math.ops import nms as hnms

    g = golden("nms_hard/wrapper")
    pre, post, thr, conf = g.np(f"a/{tag}/cfg").tolist()
    cub, sc, cat = g["a/cuboids"].to(DEV), g["a/scores"].to(DEV), g["a/categories"].to(DEV)
    want = tuple(g[f"a/{tag}/{k}"] for k in ("params", "scores", "categories", "batch_index"))
    mode = "hard" if tag == "post40" else "HARD"
    for name, got in _both_paths(lambda: hnms.batched_multiclass_nms(cub, sc, cat, int(pre), int(post), thr, conf, mode, n_classes=5)).items():
        assert got[0].device.type == "cuda"
        same_rows_exact(got, want, f"{tag} / {name}")
        _equals_restatement(got, g["a/cuboids"], g["a/scores"], g["a/categories"], (int(pre), int(post), thr, conf), f"{tag} / {name}")


def test_chain_one_sweep_and_empty_shapes_against_the_reference_wrapper(golden):
    from range_view_3d_detection_amd.math.ops import nms as hnms

    g = golden("nms_hard/wrapper")
    cub, sc, cat = g["c/cuboids"].to(DEV), g["c/scores"].to(DEV), g["c/categories"].to(DEV)
    want = (g["c/params"], g["c/scores_out"], g["c/categories_out"], g["c/batch_index"])
    for name, got in _both_paths(lambda: hnms.batched_multiclass_nms(cub, sc, cat, 50000, 1000, 0.3, 0.1, "HARD", n_classes=3)).items():
        same_rows_exact(got, want, f"chain / {name}")
        out0 = got[0].cpu()[got[2].cpu() == 0]
        has = lambda r: bool((out0 == r).all(dim=1).any())  # noqa: E731
        assert has(g["c/chain"][0]) and not has(g["c/chain"][1]) and has(g["c/chain"][2]), name  # B suppresses nothing: C is kept
    cub, sc, cat = g["a/cuboids"].to(DEV), g["a/scores"].to(DEV), g["a/categories"].to(DEV)
    m = sc[0] >= 0.1
    zero = torch.zeros(g["a/multiclass/scores"].shape[0])
    for name, (p, s, c) in _both_paths(lambda: hnms.hard_multiclass_nms(cub[0, m], sc[0, m], cat[0, m], 0.3, 50000, 40)).items():
        same_rows_exact((p, s, c, zero), (g["a/multiclass/params"], g["a/multiclass/scores"], g["a/multiclass/categories"], zero), name)
    for name, (p, s, c, b) in _both_paths(lambda: hnms.batched_multiclass_nms(cub[1:2], sc[1:2], cat[1:2], 50000, 1000, 0.3, 0.1, "HARD", n_classes=5)).items():
        assert list(p.shape) == g.np("a/empty/params_shape").tolist() and list(s.shape) == g.np("a/empty/scores_shape").tolist(), name
        assert list(c.shape) == g.np("a/empty/categories_shape").tolist() and list(b.shape) == g.np("a/empty/batch_index_shape").tolist(), name
        assert (c.dtype == torch.int64) == bool(g.np("a/empty/categories_is_int64")), name


@pytest.mark.parametrize("tag,sample", [("tiny", True), ("sampled", True), ("dense", False)])
def test_range_decoder_hard_against_the_reference(golden, tag, sample):
    """``RangeDecoder.decode(use_nms=True)`` with ``nms_mode: HARD`` from the reference's fp32 logits / regressands: ``(N,10)`` params
    with quaternions.  The candidates are decoded on the device (its sigmoid / atan2 against the CPU's): 1e-6 of max on boxes and
    scores, everything else exact."""
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder
    from test_gpu_forward import rel_err

    g = golden("nms_hard/decode")
    if tag == "tiny":
        t = golden("tiny_model")
        logits, reg, cart, mask = t["eval/logits"], t["eval/regressands"], t["cart"], t["mask"]
    else:
        t = golden("decode")
        logits, reg, cart, mask = t["logits"], t["regressands"], t["cart"], t["mask"]
    mo = {1: {"cart": cart.to(DEV), "mask": mask.to(DEV), 0: {"logits": logits.to(DEV), "regressands": reg.to(DEV)}}}
    dec = RangeDecoder(True, sample, [0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    post = {"num_pre_nms": 50000, "num_post_nms": int(g.np(f"b/{tag}/num_post_nms")), "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "HARD"}
    want = ref.canonical(*(g[f"b/{tag}/{k}"] for k in ("params", "scores", "categories", "batch_index")))
    assert want[0].shape[0] > 50 and want[0].shape[1] == 10
    for name, got in _both_paths(lambda: dec.decode(mo, post, {0: ["c"] * logits.shape[1]}, use_nms=True)).items():
        p, s, c, b = ref.canonical(*got)
        assert p.shape == want[0].shape and c.dtype == want[2].dtype and b.dtype == want[3].dtype, (tag, name, tuple(p.shape))
        assert torch.equal(c, want[2]) and torch.equal(b, want[3]), (tag, name)
        assert rel_err(p, want[0]) < 1e-6 and rel_err(s, want[1]) < 1e-6, (tag, name)


# ------------------------------------------------------------------------------------------------------------------
# 2. seeded random batches against the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.1, 0.3, 0.7])
@pytest.mark.parametrize("pre,post", [(50000, 1000), (700, 37)])
def test_clustered_batches_equal_the_restatement(thr, pre, post):
    """Classes with 0 / 1 / 63 / 64 / 65 / several thousand candidates in dense clusters (chains cross mask words and the 256-thread
    stride of the scan), score ties, a sweep of a different size; ``pre`` / ``post`` = (700, 37) cut the large classes."""
    from range_view_3d_detection_amd.math.ops import nms as hnms

    sweeps = [_clustered([0, 1, 63, 64, 65, 3000, 200, 129], 11, tie_every=7), _clustered([500, 0, 0, 4100], 12, n_centres=3, jitter=0.9),
              _clustered([64, 64, 64], 13, n_centres=1, jitter=0.3)]
    cub, sc, cat = _pad_stack(sweeps)
    cfg = (pre, post, thr, 0.1)
    args = (cub.to(DEV), sc.to(DEV), cat.to(DEV), pre, post, thr, 0.1, "HARD")
    for name, got in _both_paths(lambda: hnms.batched_multiclass_nms(*args, n_classes=8)).items():
        rows = _equals_restatement(got, cub, sc, cat, cfg, f"thr {thr} / {name}")
        assert rows > 30


def test_first_kept_box_of_a_long_chain_of_near_copies():
    """One class, 20 000 near-copies of one box plus a few far ones: one kept box suppresses words across the whole segment (every
    thread of the scan's stride has rows to fold); threshold 0.7 keeps a few hundred."""
    from range_view_3d_detection_amd.math.ops import nms as hnms

    far = _clustered([40], 22, n_centres=40, jitter=0.0, spread=4000.0)
    for thr, jitter in ((0.3, 0.2), (0.7, 0.8)):
        near = _clustered([20000], 21, n_centres=1, jitter=jitter)
        cub, sc, cat = (torch.cat([a, b])[None] for a, b in zip(near, far))
        got = hnms.batched_multiclass_nms(cub.to(DEV), sc.to(DEV), cat.to(DEV), 50000, 1000, thr, 0.1, "HARD", n_classes=1)
        _equals_restatement(got, cub, sc, cat, (50000, 1000, thr, 0.1), f"near copies, thr {thr}")


# ------------------------------------------------------------------------------------------------------------------
# 3. mask budget and capacity
# ------------------------------------------------------------------------------------------------------------------
def test_mask_budget_resume_and_capacity_overflow_give_the_same_rows():
    from range_view_3d_detection_amd.math.ops import nms as hnms

    cub, sc, cat = _pad_stack([_clustered([1500, 900, 0, 2600], 31), _clustered([300, 100], 32)])
    args = (cub.to(DEV), sc.to(DEV), cat.to(DEV), 50000, 100, 0.3, 0.1, "HARD")
    want = hnms.batched_multiclass_nms(*args, n_classes=4)
    _equals_restatement(want, cub, sc, cat, (50000, 100, 0.3, 0.1), "one pass")
    calls = []
    orig = hnms.nms_sweeps

    def spy(*a, **kw):
        out = orig(*a, **kw)
        calls.append(out[3])
        return out

    hnms.nms_sweeps = spy
    old_words, old_max = hnms.MASK_WORDS, hnms.FUSED_CLASSES_MAX
    try:
        hnms.MASK_WORDS = 1000  # sweep 0 needs ~190 000 words: the kernels report it, the host resumes over a buffer of that size
        resumed = hnms.batched_multiclass_nms(*args, n_classes=4)
        assert calls and all(c >= 0 for c in calls[-1]), calls
        hnms.MASK_WORDS = old_words
        hnms.FUSED_CLASSES_MAX = 1024  # sweep 0 has more candidates than the capacity (-2): per-class loop; sweep 1 stays on device
        calls.clear()
        overflow = hnms.batched_multiclass_nms(*args, n_classes=4)
        assert calls[0][0] == -2 and calls[0][1] >= 0, calls
    finally:
        hnms.nms_sweeps = orig
        hnms.MASK_WORDS, hnms.FUSED_CLASSES_MAX = old_words, old_max
    for what, got in (("resumed", resumed), ("capacity overflow", overflow)):
        for a, b in zip(got, want):
            assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------------------------
# 4. a full-size sweep through the decoder
# ------------------------------------------------------------------------------------------------------------------
def test_full_size_sweep_through_the_decoder_equals_the_restatement():
    """64 x 2048, band-sampled: the decoder's 212 992 candidates per sweep; a few thousand pass ``min_confidence``, neighbouring pixels
    decode to near-copies of one box.  The candidates are the device's own (``decode_candidates``), so the comparison is exact."""
    from range_view_3d_detection_amd.math.linalg.lie.SO3 import yaw_to_quat
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder, decode_candidates

    g = torch.Generator().manual_seed(5)
    B, C, H, W = 2, 5, 64, 2048
    inc = torch.linspace(0.2, -0.4, H).view(1, 1, H, 1)
    az = torch.linspace(math.pi, -math.pi, W).view(1, 1, 1, W)
    r = (20.0 + 15.0 * torch.sin(3 * az) + 10.0 * torch.cos(7 * inc) + torch.rand(B, 1, H, W, generator=g)).clamp(1.5, 80.0)
    mask = torch.rand(B, 1, H, W, generator=g) >= 0.1
    cart = (torch.cat([r * inc.cos() * az.cos(), r * inc.cos() * az.sin(), r * inc.sin().expand(B, 1, H, W)], dim=1) * mask).float()
    logits = torch.randn(B, C, H, W, generator=g) - 4.6
    reg = torch.randn(B, 8, H, W, generator=g) * torch.tensor([0.3, 0.3, 0.3, 0.1, 0.1, 0.1, 0.1, 0.0]).view(1, 8, 1, 1)
    reg[:, 3:6] += torch.tensor([4.5, 2.0, 1.7]).log().view(1, 3, 1, 1)
    reg[:, 7] = 1.0
    bands = ([0, 15, 30], [15, 30, math.inf], [8, 2, 1])
    mo = {1: {"cart": cart.to(DEV), "mask": mask.to(DEV), 0: {"logits": logits.to(DEV), "regressands": reg.to(DEV)}}}
    s, c, b = decode_candidates(mo[1][0]["logits"], mo[1][0]["regressands"], mo[1]["cart"], mo[1]["mask"], True, *bands)
    assert s.shape[1] == 212992
    n_live = int((s >= 0.1).sum())
    assert 4000 < n_live < 60000, n_live
    dec = RangeDecoder(True, True, *bands)
    post = {"num_pre_nms": 50000, "num_post_nms": 300, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "HARD"}
    p, so, co, bo = dec.decode(mo, post, {0: ["c"] * C}, use_nms=True)
    assert p.shape[1] == 10
    bi, ki, ci = ref.batched(b, s, c, 50000, 300, 0.3, 0.1)
    assert p.shape[0] == bi.size and bi.size > 500 and bi.size < n_live
    bi, ki = torch.from_numpy(bi).to(DEV), torch.from_numpy(ki).to(DEV)
    assert torch.equal(p[:, :6], b[bi, ki][:, :6]) and torch.equal(p[:, 6:], yaw_to_quat(b[bi, ki][:, -1:]))
    assert torch.equal(so, s[bi, ki]) and torch.equal(co.long().cpu(), torch.from_numpy(ci)) and torch.equal(bo.long(), bi)


# ------------------------------------------------------------------------------------------------------------------
# 5. the one-list FFI, the shim, the fp16-operand library
# ------------------------------------------------------------------------------------------------------------------
def test_rv_nms_rotated_alone_with_and_without_classes():
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.math.ops import nms as hnms

    cub, sc, cat = _clustered([700, 300, 65], 41, tie_every=5)
    order = torch.from_numpy(ref.score_order(sc.numpy()))
    rect = ref.rect_of(cub[order].numpy())
    rect_d = torch.from_numpy(rect).to(DEV)
    for thr in (0.1, 0.5):
        want = ref.nms_sorted(rect, thr)
        got = hnms.nms_rotated_sorted(rect_d, thr)
        assert got.dtype == torch.int64 and got.device.type == "cuda" and got.cpu().tolist() == want.tolist()
        with L.operand("f16"):  # the fp16-operand library exports the same entry: same rows
            assert hnms.nms_rotated_sorted(rect_d, thr).cpu().tolist() == want.tolist()
        # with classes: the union over classes of each class's own result
        per_class = sorted(int(i) for j in range(3) for i in (cat[order] == j).nonzero().flatten()[ref.nms_sorted(rect[(cat[order] == j).numpy()], thr)])
        assert hnms.nms_rotated_sorted(rect_d, thr, cats=cat[order].to(DEV)).cpu().tolist() == per_class
    assert hnms.nms_rotated_sorted(rect_d[:0], 0.3).numel() == 0
    assert hnms.nms_rotated_sorted(rect_d[:1], 0.3).cpu().tolist() == [0]


def test_detectron2_shaped_shim_on_unsorted_input_with_ties():
    from range_view_3d_detection_amd.compat.detectron2_nms import nms_rotated

    cub, sc, _ = _clustered([900], 42, tie_every=3)
    boxes = torch.cat([cub[:, [0, 1, 3, 4]], -cub[:, 6:7].rad2deg()], dim=1)  # what the reference hands to detectron2 (nms.py:33-39)
    for thr in (0.3, torch.as_tensor(0.55)):
        want = ref.nms_rotated(boxes.numpy(), sc.numpy(), float(thr))
        got = nms_rotated(boxes=boxes.to(DEV), scores=sc.to(DEV), iou_threshold=thr)
        assert got.dtype == torch.int64 and got.device.type == "cuda" and got.cpu().tolist() == want.tolist()
        assert bool((sc[got.cpu()][1:] <= sc[got.cpu()][:-1]).all()) and 5 < len(want) < 900
    assert nms_rotated(boxes[:0].to(DEV), sc[:0].to(DEV), 0.3).shape == (0,)


def test_f16_library_batch_entry_gives_the_same_rows(golden):
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.math.ops import nms as hnms

    g = golden("nms_hard/wrapper")
    args = (g["a/cuboids"].to(DEV), g["a/scores"].to(DEV), g["a/categories"].to(DEV), 50000, 40, 0.3, 0.1, "HARD")
    want = hnms.batched_multiclass_nms(*args, n_classes=5)
    with L.operand("f16"):
        got = hnms.batched_multiclass_nms(*args, n_classes=5)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 6. no shared state between the modes
# ------------------------------------------------------------------------------------------------------------------
def test_weighted_after_hard_still_equals_the_weighted_fixture(golden):
    from range_view_3d_detection_amd.math.ops import nms as hnms
    from test_gpu_nms_wrapper import _same_rows

    g = golden("nms_wrapper")
    pre, post, thr, conf = g.np("a/post40/cfg").tolist()
    cub, sc, cat = g["a/cuboids"].to(DEV), g["a/scores"].to(DEV), g["a/categories"].to(DEV)
    want = tuple(g[f"a/post40/{k}"] for k in ("params", "scores", "categories", "batch_index"))
    for _ in range(2):
        hard = hnms.batched_multiclass_nms(cub, sc, cat, int(pre), int(post), thr, conf, "HARD", n_classes=5)
        _equals_restatement(hard, g["a/cuboids"], g["a/scores"], g["a/categories"], (int(pre), int(post), thr, conf), "hard between weighted runs")
        weighted = hnms.batched_multiclass_nms(cub, sc, cat, int(pre), int(post), thr, conf, "WEIGHTED", n_classes=5)
        _same_rows(weighted, want, "weighted after hard")
