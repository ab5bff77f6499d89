"""The fixtures of ``tests/golden/loss_kinds/`` (the reference's own DetectionHead with every ``_cls_loss`` / ``_regression_loss`` pair of
``tests/golden/make_golden_loss_kinds.py``): the generator reproduces the committed directory byte for byte, and the files hold what the
cases are for.  Host side, no GPU."""

from __future__ import annotations

import os

import pytest
import torch

from test_oracle_golden import GOLDEN, unpack

DIR = os.path.join(GOLDEN, "loss_kinds")
NAMES = ["a.npz", "b.npz", "c.npz", "common.npz", "d.npz", "e.npz"]
HAVE_REFERENCE = os.path.isdir("/root/reference/src/torchbox3d")


@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: regenerating the fixtures runs the reference")
def test_generator_reproduces_the_committed_directory(tmp_path):
    """As tests/test_multilevel_golden.py does for its directory: twice, as the machine is and with ATen's scalar code paths on one thread."""
    import subprocess
    import sys

    assert sorted(os.listdir(DIR)) == NAMES
    assert sum(os.path.getsize(os.path.join(DIR, f)) for f in NAMES) < 600 * 1024
    for tag, extra in (("native", {}), ("scalar", {"ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1"})):
        out_dir = tmp_path / tag
        out_dir.mkdir()
        env = dict(os.environ, RV3D_GOLDEN_OUT=str(out_dir), PYTORCH_JIT="0", **extra)
        out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_loss_kinds.py")], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        for f in NAMES:
            assert open(os.path.join(DIR, f), "rb").read() == open(out_dir / "loss_kinds" / f, "rb").read(), f"{f} is not reproduced ({tag})"


def test_fixtures_hold_what_the_cases_are_for(golden):
    """Read from the stored tensors (the generator asserts the same on the reference's run)."""
    assert sorted(os.listdir(DIR)) == NAMES
    assert len([f for f in os.listdir(GOLDEN) if f.endswith(".npz")]) == 13, "the fixtures of the loss kinds live in their own directory"
    for name, prefixes in (("a", ["s1/t0"]), ("b", ["s1/t0", "s1/t1", "s2/t0", "s2/t1"])):
        g = golden(f"loss_kinds/{name}")
        soft = torch.cat([g[f"{p}/soft"].flatten() for p in prefixes])
        assert bool((soft == 1).any()) and bool(((soft > 0) & (soft < 1)).any()), name
    for name, thr in (("b", 0.5), ("c", 0.25), ("e", 0.5)):
        g = golden(f"loss_kinds/{name}")
        on = (g["s1/t0/classification_labels"] < g["s1/t0/logits"].shape[1])[:, None] & g["s1/mask"].bool()
        d = (g["s1/t0/regressands"] - g["s1/t0/regression_targets"]).abs()
        assert bool(((d < thr / 2) & on).any()) and bool(((d > 2 * thr) & on).any()), name
    for name in "abcde":
        assert set(unpack(golden(f"loss_kinds/{name}"), "loss")) >= {"loss", "classification_loss", "regression_loss", "total_fg", "total_objects", "loss/s1"}


@pytest.mark.skipif(not HAVE_REFERENCE, reason="build container only: imports the generator, which imports the reference")
def test_case_table_is_the_generators():
    """The configurations tests/test_gpu_loss_kinds_head.py builds its heads from are the generator's."""
    import json
    import subprocess
    import sys

    from test_gpu_loss_kinds_head import CASES

    code = ("import sys, json; sys.path.insert(0, %r); import make_golden_loss_kinds as m; "
            "print(json.dumps({k: {f: v[f] for f in ('strides', 'classes', 'method', 'partitions', 'normalize', 'cls', 'reg')} for k, v in m.CASES.items()}))" % GOLDEN)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTORCH_JIT="0"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(CASES))
