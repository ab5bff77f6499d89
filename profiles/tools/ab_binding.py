"""Per-call cost of the ctypes binding itself, on the CPU: N calls of the host-only ``rv_tap_launch_info`` / ``rv_ew_pass_info``
through ``_lib.tap_launch_info`` / ``_lib.ew_pass_info`` of this tree and of another ``_lib.py`` (a checkout of another commit), both
on this tree's library, interleaved in one process.

    python profiles/tools/ab_binding.py OTHER/range_view_3d_detection_amd/_lib.py [calls per round] [rounds]
"""

import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("RV3D_LIB", os.path.join(ROOT, "range_view_3d_detection_amd", "librv3d_hip.so"))


def _import(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    calls, rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 100000, int(sys.argv[3]) if len(sys.argv) > 3 else 9
    arms = {}
    for tag, path in (("other", sys.argv[1]), ("this", os.path.join(ROOT, "range_view_3d_detection_amd", "_lib.py"))):
        L = _import("lib_" + tag, path)
        g, s = L.TapGeom(3, 3, 1, 1, 1, 256, 256), L.TapShape(4, 64, 2048, 2048, 256, 256, L.OUT_STATS)
        arms[tag, "tap_launch_info"] = (lambda L=L, g=g, s=s: L.tap_launch_info(g, s, False)), []
        arms[tag, "ew_pass_info"] = (lambda L=L: L.ew_pass_info(L.EW_PASS_BWD_APPLY, 524288, 64, None, True, True, 0)), []
    for _ in range(rounds):
        for fn, times in arms.values():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            times.append((time.perf_counter() - t0) / calls * 1e6)
    for (tag, name), (_, times) in arms.items():
        print(f"{tag:5s} {name:16s} min {min(times):.3f}  median {sorted(times)[len(times) // 2]:.3f} us per call ({rounds} x {calls} calls, interleaved)")


if __name__ == "__main__":
    main()
