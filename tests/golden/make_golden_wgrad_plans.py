"""Fixture for the weight-gradient planner: ``tests/golden/wgrad_plans.json``.

What ``rv_tap_wgrad_info`` (kernel generation, split-K slabs, workgroups) and ``rv_tap_wgrad_workspace_bytes`` answer for a sweep of layers,
recorded from the library as built.  Both are planning entry points: they launch nothing and run without a device, where they plan for 256
compute units (an MI355X's count), so the table is the same on a box without a GPU and on an MI355X.  Record it from the commit BEFORE a
change of ``csrc/wgrad.hip`` that is meant to keep its decisions; ``test_weight_gradient_plans_equal_the_recorded_table``
(``tests/test_host_cpu.py``) then asks for every row, exactly.

``rows`` (one list of integers per call), columns ``columns``: the inputs ``kh kw stride_w pad_h pad_w cu cv N H Wu Wv flags``, then ``gen ksplit
workgroups`` (``info[0..2]``), then ``workspace_bytes``.  The sweep is the product of

* kernels (kh, kw, pad_h, pad_w): 1x1, 3x3, 3x7 and the 3x8 of the transposed convs;
* ``stride_w`` 1, 2, 4 with Wv = Wu * stride_w (strided layers stay on generation 1);
* (cu, cv): 3 and 64 / 96 channels (padded widths that are no multiple of 128: never generation 3), one to four 128-channel tiles a side,
  and the folded views' 128 <-> 512 and 256 <-> 1024;
* Wu below 64 (generation 1), 63 / 64 (the threshold), widths with a partial last chunk (200, 1808, 2656) and whole ones (512, 2048);
* a crop (N, H) = (1, 16), where the 32-chunk floor of a slice caps the split, and the training batch (4, 64);
* plain operands and the folded BatchNorm + ReLU on the way in (generation 2 instead of 3).

The recorder refuses a table that does not hold all three generations, or no balanced split (``ksplit * tiles * groups != workgroups``:
the remainder workgroups of the 48-tile layers).
"""

from __future__ import annotations

import ctypes
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from range_view_3d_detection_amd import _lib  # noqa: E402

OUT = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "wgrad_plans.json")
COLUMNS = ["kh", "kw", "stride_w", "pad_h", "pad_w", "cu", "cv", "N", "H", "Wu", "Wv", "flags", "gen", "ksplit", "workgroups", "workspace_bytes"]

KERNELS = [(1, 1, 0, 0), (3, 3, 1, 1), (3, 7, 1, 3), (3, 8, 1, 2)]
STRIDES = [1, 2, 4]
CHANNELS = [(3, 64), (64, 64), (64, 96), (128, 128), (256, 256), (512, 512), (128, 512), (256, 1024)]
WIDTHS = [32, 63, 64, 200, 512, 1808, 2048, 2656]
BATCHES = [(1, 16), (4, 64)]
FLAGS = [0, _lib.IN_AFFINE | _lib.IN_RELU]


def sweep():
    """The inputs of every call, in a fixed order."""
    for (kh, kw, ph, pw), st, (cu, cv), wu, (n, h), flags in itertools.product(KERNELS, STRIDES, CHANNELS, WIDTHS, BATCHES, FLAGS):
        yield kh, kw, st, ph, pw, cu, cv, n, h, wu, wu * st, flags


def answer(handle, row):
    """``(gen, ksplit, workgroups, workspace_bytes)`` of one call; both entry points must accept it."""
    kh, kw, st, ph, pw, cu, cv, n, h, wu, wv, flags = (int(v) for v in row)
    g, s = _lib.TapGeom(kh, kw, st, ph, pw, cu, cv), _lib.TapShape(n, h, wu, wv, 0, 0, flags)
    info = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    rc = handle.rv_tap_wgrad_info(ctypes.byref(g), ctypes.byref(s), info)
    assert rc == 0, (row, handle.rv_last_error())
    nbytes = handle.rv_tap_wgrad_workspace_bytes(ctypes.byref(g), ctypes.byref(s))
    assert nbytes > 0, row
    return info[0], info[1], info[2], nbytes


def tiles_times_groups(row):
    """128 x 128 channel tiles x groups of up to three taps of a kernel row: the workgroups of ONE K slice of generations 2 / 3."""
    kh, kw, cu, cv = int(row[0]), int(row[1]), int(row[5]), int(row[6])
    pad32 = lambda c: (c + 31) & ~31  # noqa: E731
    return -(-pad32(cu) // 128) * -(-pad32(cv) // 128) * kh * ((kw + 2) // 3)


def main() -> None:
    handle = _lib.load()
    rows = np.array([inp + answer(handle, inp) for inp in sweep()], dtype=np.int64)
    gen, ksplit, wgs = rows[:, 12], rows[:, 13], rows[:, 14]
    per_gen = {g: int((gen == g).sum()) for g in (1, 2, 3)}
    balanced = [r for r in rows if r[12] == 3 and r[13] * tiles_times_groups(r) != r[14]]
    print(f"{len(rows)} rows; generation 1 / 2 / 3: {per_gen[1]} / {per_gen[2]} / {per_gen[3]}; split-K factors {ksplit.min()} .. {ksplit.max()}, "
          f"workgroups {wgs.min()} .. {wgs.max()}")
    print(f"check 1 (rows of all three generations): {'ok' if all(per_gen.values()) else 'FAILED'}")
    print(f"check 2 (a balanced split, ksplit * tiles * groups != workgroups): {'ok' if balanced else 'FAILED'}: {len(balanced)} rows, the first "
          f"{dict(zip(COLUMNS, (int(v) for v in balanced[0]))) if balanced else None}")
    assert all(per_gen.values()) and balanced and set(gen.tolist()) == {1, 2, 3}
    with open(OUT, "w") as f:
        json.dump({"compute_units": 256, "columns": COLUMNS, "rows": rows.tolist()}, f, separators=(",", ":"))
        f.write("\n")
    print(f"wgrad_plans.json: {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
