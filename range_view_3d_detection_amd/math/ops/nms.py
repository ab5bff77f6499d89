"""Multi-class NMS, ``nms_mode`` WEIGHTED and HARD -- mirrors ``torchbox3d/math/ops/nms.py:10-266``.

``weighted_nms`` keeps the reference wrapper's signature and contract around the op-level FFI
``weighted_nms_ext.wnms_gpu`` (``nms.py:126-177``); here that FFI is ``rv_wnms`` of
``librv3d_hip.so``.  The kernel's arithmetic is not in the reference tree (third-party, un-pinned):
the semantics implemented are declared in ``DESIGN.md`` / ``oracle/nms.py`` -- parity unpinned.

``hard_multiclass_nms`` is the reference's function of that name (``nms.py:10-61``) around ``detectron2.layers.nms.nms_rotated``;
here that call is ``rv_nms_rotated`` (declared semantics in ``include/rv3d.h``: descending score, ties by ascending index, a kept
box suppresses later boxes with rotated BEV IoU strictly above the threshold).  Hard NMS is a selection: every output row is
an input row, bit for bit.

``WnmsSemantics`` names the four free choices of the weighted-NMS declaration (``RV_WNMS_*`` of ``include/rv3d.h``); every
weighted entry here takes it as ``semantics=None`` (None: the declaration) and passes it per call -- there is no option state.
"""

from __future__ import annotations

import ctypes
import dataclasses
import functools
import math
from typing import Any, List, Mapping, Optional, Tuple

import torch
from torch import Tensor

from ... import _lib as L
from ...engine import _require_cuda


# field -> (the declaration's value, the other reading, the RV_WNMS_* flag the other reading sets)
_WNMS_CHOICES = {"merge_set": ("ALIVE", "ALL", L.WNMS_MERGE_SUPPRESSED), "score": ("MEAN", "KEEPER", L.WNMS_SCORE_KEEPER),
                 "nms_compare": ("GT", "GE", L.WNMS_NMS_GE), "merge_compare": ("GT", "GE", L.WNMS_MERGE_GE)}


@dataclasses.dataclass(frozen=True)
class WnmsSemantics:
    """The four free choices of the weighted-NMS declaration (``oracle/nms.py``) -- the axes along which a third-party
    ``wnms_gpu`` may differ from it.  The defaults are the declaration.

    ``merge_set``      ``ALIVE``: a cluster takes the later boxes not yet suppressed when its keeper is visited; ``ALL``: every
                       later box of the class that passes the merge test (a box may be in several clusters).
    ``score``          ``MEAN``: the score column of an output row is the weighted mean like the others; ``KEEPER``: the keeper's own score.
    ``nms_compare``    ``GT``: suppressed when ``iou > nms_thresh``; ``GE``: when ``iou >= nms_thresh``.
    ``merge_compare``  ``GT`` / ``GE``: the same for ``merge_thresh``.
    """

    merge_set: str = "ALIVE"
    score: str = "MEAN"
    nms_compare: str = "GT"
    merge_compare: str = "GT"

    def __post_init__(self) -> None:
        for name, (default, other, _) in _WNMS_CHOICES.items():
            value = getattr(self, name)
            up = value.upper() if isinstance(value, str) else value
            if up not in (default, other):
                raise L.RvError(f"wnms_semantics: {name} = {value!r} is not one of {default!r}, {other!r}")
            object.__setattr__(self, name, up)

    @property
    def flags(self) -> int:
        """The ``RV_WNMS_*`` bits of this setting (0: the declaration)."""
        return sum(flag for name, (_, other, flag) in _WNMS_CHOICES.items() if getattr(self, name) == other)

    @classmethod
    def from_flags(cls, flags: int) -> "WnmsSemantics":
        """The inverse of ``.flags``: the setting of a set of ``RV_WNMS_*`` bits (public: ``tests/tools/pin_wnms.py`` enumerates the 16
        settings with it)."""
        return cls(**{name: (other if flags & flag else default) for name, (default, other, flag) in _WNMS_CHOICES.items()})

    @classmethod
    def from_config(cls, config: Optional[Mapping[str, Any]]) -> "WnmsSemantics":
        """From a ``wnms_semantics:`` block (a Hydra ``DictConfig`` or a plain dict; ``None``: the declaration)."""
        if config is None:
            return cls()
        if not hasattr(config, "keys"):
            raise L.RvError(f"wnms_semantics: expected a mapping, got {type(config).__name__}")
        unknown = sorted(str(k) for k in config.keys() if k not in _WNMS_CHOICES)
        if unknown:
            raise L.RvError(f"wnms_semantics: unknown option(s) {unknown}; the options are {sorted(_WNMS_CHOICES)}")
        return cls(**{str(k): config[k] for k in config.keys()})


def _flags(semantics: Optional[WnmsSemantics]) -> int:
    if semantics is None:
        return 0
    if not isinstance(semantics, WnmsSemantics):
        raise L.RvError(f"semantics must be a WnmsSemantics or None, got {type(semantics).__name__}")
    return semantics.flags


def wnms_sorted(boxes: Tensor, data: Tensor, output: Tensor, keep: Tensor, count: Tensor, nms_threshold: float, merge_thresh: float,
                semantics: Optional[WnmsSemantics] = None, cats: Optional[Tensor] = None) -> int:
    """The ``rv_wnms`` call: score-sorted contiguous f32 device ``boxes`` (N,5) and ``data`` (N,C+1, last column the score); fills
    rows ``[0, k)`` of ``output`` (N,C+1), ``keep`` and ``count`` (int64, device) and returns k (synchronous).  A non-default
    ``semantics`` goes through ``rv_wnms_opt``.  ``cats`` (public, optional): a contiguous int32 device tensor with a class per box --
    boxes of different classes neither suppress nor merge; it is the ``cats`` argument of ``rv_wnms_opt`` / ``rv_wnms_classes``, which
    had no Python caller before, and also goes through ``rv_wnms_opt``."""
    n, d = data.shape
    flags = _flags(semantics)
    ws = torch.empty(L.load().rv_wnms_workspace_bytes(n), dtype=torch.uint8, device=boxes.device)
    num_out = ctypes.c_int64(0)
    if flags == 0 and cats is None:
        L.call("rv_wnms", L.ptr(boxes), L.ptr(data), n, d, nms_threshold, merge_thresh, L.ptr(output),
               L.ptr(keep), L.ptr(count), L.ptr(ws), ctypes.byref(num_out), L.stream_ptr())
    else:
        L.call("rv_wnms_opt", L.ptr(boxes), L.ptr(data), L.ptr(cats), n, d, nms_threshold, merge_thresh, L.ptr(output),
               L.ptr(keep), L.ptr(count), L.ptr(ws), ctypes.byref(num_out), L.stream_ptr(), flags)
    return int(num_out.value)


def weighted_nms(boxes: Tensor, data2merge: Tensor, scores: Tensor, nms_threshold: float, merge_thresh: float,
                 semantics: Optional[WnmsSemantics] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """boxes (N,5) [x1,y1,x2,y2,ry], data2merge (N,C), scores (N,) -> (keep indices, merged rows (K,C+1), counts (K,))."""
    _require_cuda(boxes, "boxes")
    sorted_scores, order = scores.sort(0, descending=True)
    boxes = boxes[order].contiguous().float()
    data = torch.cat([data2merge[order].float(), sorted_scores[:, None].float()], 1).contiguous()
    output = torch.zeros_like(data)
    keep = torch.zeros(data.shape[0], dtype=torch.long, device=boxes.device)
    count = torch.zeros(data.shape[0], dtype=torch.long, device=boxes.device)
    k = wnms_sorted(boxes, data, output, keep, count, nms_threshold, merge_thresh, semantics)
    return order[keep[:k]].contiguous(), output[:k], count[:k]


# Device-resident path (``rv_nms_sweeps``, csrc/nms2.hip): all sweeps of a batch in one set of launches, one device->host
# read at the end.  The per-candidate arrays are sized for every candidate of the sweep (up to ``FUSED_CLASSES_MAX``; the
# decoder emits 212 992 per 64 x 2048 sweep); the class-relative pair masks get a word budget (``MASK_WORDS`` per sweep and
# mask: 32 MB each), and a batch in which some sweep needs more -- tens of thousands of candidates in ONE class -- is redone
# over a buffer of the size the kernels report (second read; the ordering stages are not repeated).  The reference's
# per-class pre-NMS cut (``topk(num_pre_nms)``, nms.py:83-84) is applied on device.  Only a sweep with more candidates than
# ``FUSED_CLASSES_MAX`` (or more than 64 classes) takes the reference-shaped per-class loop over the FFI below.
FUSED_CLASSES_MAX = 262144
MASK_WORDS = 4 * 1024 * 1024
NMS_MODES = ("WEIGHTED", "HARD")


def _check_mode(nms_mode: str) -> str:
    mode = nms_mode.upper()
    if mode not in NMS_MODES:
        raise NotImplementedError(f"NMS Mode: {mode} is not implemented.")  # (the reference's message, nms.py:240)
    return mode


def _check_semantics(nms_mode: str, semantics: Optional[WnmsSemantics]) -> None:
    """HARD with a non-default setting is refused: the options describe weighted NMS only."""
    if _flags(semantics) != 0 and nms_mode.upper() == "HARD":
        raise L.RvError(f"nms_mode HARD takes no wnms_semantics (the options describe weighted NMS only), got {semantics}")


def nms_sweeps(cuboids: Tensor, scores: Tensor, categories: Tensor, n_classes: int, iou_threshold: float, min_confidence: float,
               num_post_nms: int, cap: int, num_pre_nms: int = 2**31 - 1, mode: str = "WEIGHTED",
               semantics: Optional[WnmsSemantics] = None) -> Tuple[Tensor, Tensor, Tensor, List[int]]:
    """(B,K,7), (B,K), (B,K) -> padded (B,R,7) boxes, (B,R) scores, (B,R) int32 classes and the per-sweep row counts
    (-2: the sweep had more than ``cap`` candidates -- its rows are not valid).  ``mode`` HARD: ``rv_nms_sweeps_hard`` -- one pair
    mask per sweep instead of two, rows copied from the inputs.  A non-default ``semantics``: ``rv_nms_sweeps_opt``."""
    _check_semantics(mode, semantics)
    _require_cuda(cuboids, "cuboids")
    hard = _check_mode(mode) == "HARD"
    flags = _flags(semantics)
    dev = cuboids.device
    B, K, _ = cuboids.shape
    cub = cuboids.detach().float().contiguous()
    sc = scores.detach().float().contiguous()
    ct = categories.detach().to(torch.int64).contiguous()
    out_cap = min(cap, n_classes * num_post_nms)
    ob = torch.empty((B, out_cap, 7), dtype=torch.float32, device=dev)
    os_ = torch.empty((B, out_cap), dtype=torch.float32, device=dev)
    oc = torch.empty((B, out_cap), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int64, device=dev)
    ws = torch.empty(L.load().rv_nms_sweeps_workspace_bytes(B, cap), dtype=torch.uint8, device=dev)
    num_pre = int(min(num_pre_nms, 2**31 - 1))

    def run(mask_words: int, resume: int) -> List[List[int]]:
        masks = torch.empty((B, 1 if hard else 2, mask_words), dtype=torch.int64, device=dev)
        head = (L.ptr(sc), L.ptr(ct), L.ptr(cub), B, K, n_classes, min_confidence, iou_threshold)
        tail = (num_pre, num_post_nms, cap, out_cap, L.ptr(ob), L.ptr(os_), L.ptr(oc), L.ptr(counts), L.ptr(ws),
                L.ptr(masks), mask_words, resume, L.stream_ptr())
        if hard:
            L.call("rv_nms_sweeps_hard", *head, *tail)
        elif flags == 0:
            L.call("rv_nms_sweeps", *head, 0.5, *tail)
        else:
            L.call("rv_nms_sweeps_opt", *head, 0.5, *tail, flags)
        return counts.tolist()  # the one device->host read of the batch (a second one only when the mask budget was exceeded)

    budget = int(min(MASK_WORDS, max(1, (cap // 64 + 1) * cap)))  # (small inputs: no more than one class could need)
    rows = run(budget, 0)
    if any(r[0] == -1 for r in rows):
        rows = run(max(r[3] for r in rows), 1)
    return ob, os_, oc, [int(r[0]) for r in rows]


def _capacity(k: int) -> int:
    return max(64, (min(k, FUSED_CLASSES_MAX) + 63) // 64 * 64)


def nms_rotated_sorted(boxes: Tensor, iou_threshold: float, cats: Tensor = None) -> Tensor:
    """``rv_nms_rotated``: rectangles (n,5) [x1,y1,x2,y2,ry] SORTED by score descending (``cats``: optional class per box, boxes of
    different classes do not interact) -> sorted positions of the kept boxes, ascending, int64 on the device."""
    _require_cuda(boxes, "boxes")
    b = boxes.detach().float().contiguous()
    n = b.shape[0]
    c = None if cats is None else cats.detach().to(torch.int32).contiguous()
    keep = torch.empty(n, dtype=torch.long, device=b.device)
    ws = torch.empty(L.load().rv_nms_rotated_workspace_bytes(n), dtype=torch.uint8, device=b.device)
    num_out = ctypes.c_int64(0)
    L.call("rv_nms_rotated", L.ptr(b), L.ptr(c), n, iou_threshold, L.ptr(keep), L.ptr(ws), ctypes.byref(num_out), L.stream_ptr())
    return keep[: int(num_out.value)]


def _multiclass_nms(mode: str, cuboids_i: Tensor, scores_i: Tensor, categories_i: Tensor, iou_threshold: float, num_pre_nms: int,
                    num_post_nms: int, semantics: Optional[WnmsSemantics] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """One sweep: the device-resident path when it fits, else per class (ascending ``unique``) top-k pre, NMS over the list FFI,
    top-k post."""
    n = scores_i.shape[0]
    if 0 < n <= FUSED_CLASSES_MAX:
        n_cls = int(categories_i.max().item()) + 1
        if n_cls <= 64:
            b, s, c, cnt = nms_sweeps(cuboids_i[None], scores_i[None], categories_i[None], n_cls, iou_threshold, -math.inf, num_post_nms, _capacity(n),
                                      num_pre_nms, mode=mode, semantics=semantics)
            return b[0, : cnt[0]], s[0, : cnt[0]], c[0, : cnt[0]].to(s.dtype)
    rows: List[Tuple[Tensor, Tensor, Tensor]] = []
    for j in categories_i.unique():
        sel = categories_i == j
        s, b = scores_i[sel], cuboids_i[sel]
        k = min(len(s), num_pre_nms)
        if mode == "HARD":
            # (``topk`` leaves the order of equal scores open; the declared rule is ascending index: a stable sort)
            s, rank = s.sort(dim=0, descending=True, stable=True)
            s, rank = s[:k], rank[:k]
        else:
            s, rank = s.topk(k=k, dim=0)
        b = b[rank]
        half = b[:, 3:5] / 2
        rect = torch.cat([b[:, :2] - half, b[:, :2] + half, b[:, 6:7]], dim=-1)
        if mode == "HARD":
            keep = nms_rotated_sorted(rect, iou_threshold)[:num_post_nms]  # kept rows are in descending score order: top-k = prefix
            b, s = b[keep], s[keep]
        else:
            data = torch.cat([b[:, :6], b[:, 6:7].sin(), b[:, 6:7].cos()], dim=1)
            _, merged, _ = weighted_nms(rect, data, s, nms_threshold=iou_threshold, merge_thresh=0.5, semantics=semantics)
            box6, sn, cs, sc = merged.split([6, 1, 1, 1], dim=1)
            b = torch.cat([box6, torch.atan2(sn, cs)], dim=1)
            s, rank = sc.flatten().topk(k=min(len(b), num_post_nms), dim=0)
            b = b[rank]
        rows.append((b, s, torch.full_like(s, fill_value=float(j))))
    return tuple(torch.cat(col) for col in zip(*rows))


def weighted_multiclass_nms(cuboids_i: Tensor, scores_i: Tensor, categories_i: Tensor, iou_threshold: float, num_pre_nms: int,
                            num_post_nms: int, semantics: Optional[WnmsSemantics] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Per class (ascending ``unique``): top-k pre, weighted NMS with merge threshold 0.5 (``nms.py:105-106``), top-k post."""
    return _multiclass_nms("WEIGHTED", cuboids_i, scores_i, categories_i, iou_threshold, num_pre_nms, num_post_nms, semantics)


def hard_multiclass_nms(cuboids_i: Tensor, scores_i: Tensor, categories_i: Tensor, iou_threshold: float, num_pre_nms: int,
                        num_post_nms: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Per class (ascending ``unique``): top-k pre, hard rotated NMS, top-k post (``nms.py:10-61``); rows are input rows."""
    return _multiclass_nms("HARD", cuboids_i, scores_i, categories_i, iou_threshold, num_pre_nms, num_post_nms)


def batched_multiclass_nms(cuboids: Tensor, scores: Tensor, categories: Tensor, num_pre_nms: int, num_post_nms: int,
                           iou_threshold: float, min_confidence: float, nms_mode: str, n_classes: int = None,
                           semantics: Optional[WnmsSemantics] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Per sweep: ``score >= min_confidence`` filter, then per-class NMS (``nms.py:181-266``).  ``semantics``: the weighted-NMS
    choices, on the device-resident path and in the per-class loop alike (HARD takes none)."""
    nms_mode = _check_mode(nms_mode)
    _check_semantics(nms_mode, semantics)
    multiclass_nms = hard_multiclass_nms if nms_mode == "HARD" else functools.partial(weighted_multiclass_nms, semantics=semantics)
    bs, ss, cs, ids = [], [], [], []
    B, K = scores.shape
    fast = None
    cap = _capacity(K)
    if FUSED_CLASSES_MAX > 0 and n_classes is not None and n_classes <= 64:
        # device-resident path for the whole batch; sweeps that overflow its capacity fall through to the loop below
        fast = nms_sweeps(cuboids, scores, categories, n_classes, iou_threshold, min_confidence, num_post_nms, cap, num_pre_nms, mode=nms_mode,
                          semantics=semantics)
    for i in range(B):
        if fast is not None and fast[3][i] >= 0:
            k = fast[3][i]
            if k == 0:
                continue
            b, s, c = fast[0][i, :k], fast[1][i, :k], fast[2][i, :k].to(scores.dtype)
            bs.append(b)
            ss.append(s)
            cs.append(c)
            ids.append(torch.full_like(s, fill_value=float(i)))
            continue
        m = scores[i] >= min_confidence
        if not bool(m.any()):
            continue
        b, s, c = multiclass_nms(cuboids[i, m], scores[i, m], categories[i, m], iou_threshold, num_pre_nms, num_post_nms)
        bs.append(b)
        ss.append(s)
        cs.append(c)
        ids.append(torch.full_like(s, fill_value=float(i)))
    if not bs:
        return (cuboids.new_empty((0, cuboids.shape[-1])), scores.new_empty((0, 1)), categories.new_empty((0, 1)), categories.new_empty((0, 1)))
    return torch.cat(bs), torch.cat(ss), torch.cat(cs), torch.cat(ids)
