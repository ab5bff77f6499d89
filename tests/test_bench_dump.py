"""``bench.py --dump-outputs DIR``: what the last timed step handed to its caller, as ``DIR/<name>.npy``, comparable between two builds.

* host: the writer itself (names, dtypes, the seeded samples of large arrays, the size limit);
* GPU: the arrays belong to the LAST TIMED step (not to the untimed passes behind it), are the same from run to run, and ``--steps``
  sets how many steps were timed."""

from __future__ import annotations

import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_names_dtypes_and_seeded_samples(tmp_path, monkeypatch):
    import bench

    backbone, head = bench.build_model("c16", 5)
    model = bench.Detector(backbone, head)
    g = torch.Generator().manual_seed(0)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    opt = types.SimpleNamespace(last_grad_norm=torch.tensor(3.0))
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 500)
    info = bench.dump_outputs(str(tmp_path / "a"), torch.tensor(1.5), model, opt)
    a = _load(tmp_path / "a")
    names = {f"param.{n}" for n, _ in model.named_parameters()} | {f"grad.{n}" for n, _ in model.named_parameters()} \
        | {f"buffer.{n}" for n, _ in model.named_buffers()} | {"loss", "grad_norm"}
    assert set(a) == names and info["arrays"] == len(names)
    assert float(a["loss"]) == 1.5 and float(a["grad_norm"]) == 3.0
    assert {v.dtype for v in a.values()} == {np.dtype("float32"), np.dtype("float64")}  # (float64: the integer num_batches_tracked)
    assert info["bytes"] == sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    params = dict(model.named_parameters())
    large = [n for n, p in params.items() if p.numel() > 500]
    assert large and info["sampled"] == 2 * len(large)
    for n, p in params.items():
        if p.numel() <= 500:  # small arrays whole, in their own shape
            assert np.array_equal(a[f"param.{n}"], p.detach().numpy()) and np.array_equal(a[f"grad.{n}"], p.grad.numpy())
        else:
            assert a[f"param.{n}"].shape == a[f"grad.{n}"].shape == (500,)
    # the sample is a property of the array's NAME and size, not of its values: shift every parameter by one and the same elements come back
    with torch.no_grad():
        for p in model.parameters():
            p += 1.0
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(1.5), model, opt)
    b = _load(tmp_path / "b")
    for n in params:
        assert np.allclose(b[f"param.{n}"] - a[f"param.{n}"], 1.0, atol=1e-6), n
        assert np.array_equal(b[f"grad.{n}"], a[f"grad.{n}"]), n
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    with pytest.raises(RuntimeError, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path / "c"), torch.tensor(1.5), model, opt)


def _bench(out_dir, steps, extra=()):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--widths", "c32", "--width", "512",
           "--height", "16", "--batch", "2", "--classes", "5", "--no-cpu-baseline", "--dump-outputs", str(out_dir), *extra]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["steps"] == steps and j["outputs_dumped"]["dir"] == str(out_dir)
    return j, _load(out_dir)


@pytest.mark.gpu
def test_dump_is_the_last_timed_step_and_steps_sets_the_timed_steps(tmp_path):
    """Three runs of the same seeded configuration: two timed steps with nothing behind them (the plain run), two timed steps
    followed by bench.py's untimed passes (``--full``: six more optimizer steps, the dump must not see them), and three timed steps."""
    ja, a = _bench(tmp_path / "a", 2)
    jb, b = _bench(tmp_path / "b", 2, ["--full"])
    jc, c = _bench(tmp_path / "c", 3)
    # the passes that take steps of their own ran behind --full and nowhere else
    assert jb["kernels_isolated"] and jb["roofline_hbm"]["per_entry_point"] and jb["roofline"]["isolated"]["launches"] > 0
    assert not {"kernels_isolated", "roofline_hbm", "roofline", "cpu_baseline", "forward_only", "rv_waymo", "loss_first_step"} & (set(ja) | set(jc))
    assert ja["value"] > 0 and ja["unit"] == "sweeps/s" and ja["higher_is_better"] is True and ja["dtype"] == "bf16" and ja["ms_per_step"] > 0
    assert set(a) == set(b) == set(c) and "loss" in a and any(k.startswith("grad.") for k in a) and any(k.startswith("param.") for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert float(a["loss"]) == pytest.approx(ja["config"]["loss"], rel=1e-6)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
        # same arguments, same inputs, same step count: the same arrays whatever ran after the timed region
        scale = float(np.abs(a[k]).max()) or 1.0
        assert float(np.abs(a[k] - b[k]).max()) <= 1e-6 * scale, (k, float(np.abs(a[k] - b[k]).max()), scale)
    # one more timed step is one more AdamW update of every parameter, and half as many launches again inside the timed region
    moved = [k for k in a if k.startswith("param.") and k.endswith("weight") and not np.array_equal(a[k], c[k])]
    assert moved
    counters = [k for k in a if k.endswith("num_batches_tracked")]
    assert counters and all(a[k] == 3 and b[k] == 3 and c[k] == 4 for k in counters)  # warm-up + timed steps, nothing more
    for name, row in ja["kernels"].items():
        assert 2 * jc["kernels"][name]["launches"] == 3 * row["launches"], name
