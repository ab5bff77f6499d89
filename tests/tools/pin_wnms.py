"""Which of the 16 ``WnmsSemantics`` settings is a given ``wnms_gpu``?

``oracle/nms.py`` declares the weighted-NMS semantics because TorchEx's kernel is not in the reference tree; the declaration holds
four free choices (``WnmsSemantics``).  ``identify`` feeds a fixed set of probe lists to any callable with TorchEx's signature

    wnms_gpu(boxes, data2merge_score, output, keep, count, nms_thresh, merge_thresh, device_index) -> num_out

and returns every setting whose numpy restatement (``tests/wnms_semantics_ref.py``) gives the same answer on every probe: ``keep`` and
``count`` exactly, ``output`` to 1e-5 relative.  The tolerance belongs to this tool -- a foreign kernel's summation order is unknown --
and is no test tolerance of the project, whose own kernels equal the restatement bit for bit.  The probes separate all 16 settings:
one matching setting pins the callable, none means it differs from the declaration along another axis.

    python tests/tools/pin_wnms.py

imports ``weighted_nms_ext`` at top level -- this package's own shim lives inside the package (``compat/``), so only an installed
TorchEx answers -- and prints the matching settings.  Without TorchEx it says so and exits 0.  It installs nothing and looks nowhere else.
"""

from __future__ import annotations

import functools
import os
import sys
from typing import Callable, List, Tuple

import numpy as np
import torch

_TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_TESTS, os.path.dirname(_TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import wnms_semantics_ref as ref  # noqa: E402
from range_view_3d_detection_amd.math.ops.nms import WnmsSemantics  # noqa: E402

OUTPUT_RTOL = 1e-5


@functools.lru_cache(maxsize=None)
def probes() -> List[Tuple[str, np.ndarray, np.ndarray, float, float]]:
    """(name, sorted boxes (n,5), data (n,9), nms_thresh, merge_thresh).  What separates the settings:
    merge set     -- ``chain``: the box B that keeper A suppressed is counted in keeper C's cluster too, or not;
    score column  -- every cluster of two or more (``chain``, ``scores``, ``random``): the last column is the mean or the keeper's score;
    nms compare   -- ``thresholds``: a pair at IoU == fp32(0.3) is one row or two;
    merge compare -- ``thresholds``: a pair at IoU == 0.5 is a cluster of two or of one; ``equal``: one pair at both thresholds."""
    chain, thr, sc = ref.chain_list(), ref.threshold_list(), ref.score_list()
    rnd = ref.random_list(200, 7)
    return [("chain", chain[0], chain[1], 0.3, 0.5), ("thresholds", thr[0], thr[1], 0.3, 0.5), ("equal", thr[0], thr[1], 0.5, 0.5),
            ("scores", sc[0], sc[1], 0.3, 0.5), ("random", rnd[0], rnd[1], 0.3, 0.5)]


def run(wnms_gpu: Callable, device, boxes: np.ndarray, data: np.ndarray, nms_thresh: float, merge_thresh: float):
    """One call in the reference wrapper's way (``math/ops/nms.py:161-174``): zeroed ``output``, ``keep`` on the host."""
    dev = torch.device(device)
    b = torch.from_numpy(boxes).to(dev).contiguous()
    d = torch.from_numpy(data).to(dev).contiguous()
    output = torch.zeros_like(d)
    keep = torch.zeros(d.shape[0], dtype=torch.long)
    count = torch.zeros(d.shape[0], dtype=torch.long, device=dev)
    k = int(wnms_gpu(b, d, output, keep, count, nms_thresh, merge_thresh, dev.index))
    return keep[:k].numpy(), output[:k].cpu().numpy(), count[:k].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _expected(probe: int, flags: int):
    """The restatement's answer to probe ``probe`` under the setting with these flags (computed once per process)."""
    _, boxes, data, nms_t, merge_t = probes()[probe]
    return ref.wnms_sorted(boxes, data, nms_t, merge_t, WnmsSemantics.from_flags(flags))


def identify(wnms_gpu: Callable, device) -> List[WnmsSemantics]:
    """Every setting whose restatement matches ``wnms_gpu`` on all probes."""
    alive = list(ref.ALL_SETTINGS)
    for p, (_, boxes, data, nms_t, merge_t) in enumerate(probes()):
        keep, out, count = run(wnms_gpu, device, boxes, data, nms_t, merge_t)
        still = []
        for s in alive:
            rk, ro, rc = _expected(p, s.flags)
            if np.array_equal(keep, rk) and np.array_equal(count, rc) and ro.shape == out.shape and \
                    bool(np.all(np.abs(out.astype(np.float64) - ro) <= OUTPUT_RTOL * np.abs(ro.astype(np.float64)))):
                still.append(s)
        alive = still
    return alive


def main() -> int:
    try:
        import weighted_nms_ext  # TorchEx: top level only
    except ImportError as e:
        print(f"pin_wnms: no top-level weighted_nms_ext (TorchEx) in this environment ({e}); nothing to pin -- parity stays unpinned")
        return 0
    if not torch.cuda.is_available():
        print("pin_wnms: weighted_nms_ext is importable but there is no GPU to run wnms_gpu on")
        return 0
    found = identify(weighted_nms_ext.wnms_gpu, "cuda:0")
    print(f"pin_wnms: {weighted_nms_ext.__file__}: {len(found)} of 16 settings match")
    for s in found:
        print(f"  {s}  (flags {s.flags})")
    if not found:
        print("  none: this wnms_gpu differs from the declaration along an axis the four options do not cover")
    return 0


if __name__ == "__main__":
    sys.exit(main())
