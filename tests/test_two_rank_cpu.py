"""CPU side of the two-rank tests: the launcher's failure handling (tests/two_rank.py ``launch`` with the worker's ``cpu`` mode), and the
recorded yardstick of tests/test_gpu_two_rank.py (tests/golden/two_rank_yardstick.json, written by
``tests/tools/emulation_yardstick.py two-rank``) with its control of the inputs' discriminating power."""

from __future__ import annotations

import math
import time

import pytest
import torch

import two_rank as tr


def test_a_rank_that_dies_ends_the_launch_at_once(tmp_path):
    """Rank 1 leaves with status 3 after the rendezvous while rank 0 enters an all-reduce: the parent reports the exit with the tail of the
    output, kills what is left and returns long before its own limit (120 s) and the workers' collective timeout (60 s)."""
    t0 = time.monotonic()
    with pytest.raises(tr.TwoRankFailure) as failure:
        tr.launch("cpu", 2, tmp_path, ["--fail-rank", "1"], limit_s=120.0)
    assert time.monotonic() - t0 < 45.0
    text = str(failure.value)
    assert "exited with" in text and "leaving with status 3" in text and "nothing else is started" in text
    assert not (tmp_path / "rank1.pt").exists()


def test_two_cpu_ranks_round_trip_their_result_files(tmp_path):
    res = tr.launch("cpu", 2, tmp_path, limit_s=120.0)
    want = torch.arange(4, dtype=torch.float64) * 2 + 10.0
    assert [r["rank"] for r in res] == [0, 1] and all(torch.equal(r["sum"], want) for r in res)
    one = tr.launch("cpu", 1, tmp_path, limit_s=120.0)
    assert len(one) == 1 and torch.equal(one[0]["sum"], torch.arange(4, dtype=torch.float64))


def test_gradient_metrics_see_direction_and_scale():
    g = torch.Generator().manual_seed(0)
    ref = {"a": torch.randn(8, 4, generator=g), "b": torch.randn(16, generator=g), "dead": torch.zeros(3)}
    same = tr.grad_metrics({k: v.clone() for k, v in ref.items()}, ref)
    assert same["parameters"] == 2 and abs(same["median"] - 1.0) < 1e-12 and same["lr_max"] < 1e-12
    doubled = tr.grad_metrics({k: 2.0 * v for k, v in ref.items()}, ref)  # cosine cannot see a factor of the world size; the norm ratio does
    assert abs(doubled["min"] - 1.0) < 1e-12 and abs(doubled["lr_q95"] - math.log(2.0)) < 1e-12
    flipped = tr.grad_metrics({"a": -ref["a"], "b": ref["b"], "dead": ref["dead"]}, ref)
    assert flipped["min"] == pytest.approx(-1.0) and flipped["worst"][0][0] == "a"


CASE_KEYS = [tr.case_key(name, shift) for name, spec in tr.CASES.items() for shift in spec[6]]


@pytest.mark.parametrize("key", CASE_KEYS)
def test_recorded_yardstick_and_its_local_batchnorm_control(key):
    """The emulation itself meets the criteria the device runs are held to, and the CONTROL -- the fp32 oracle run per rank slice with local
    BatchNorm, gradients summed: what a rank-local SyncBN computes -- misses them by a clear margin, so the inputs can tell the two apart.

    Clear margin: the realisations of the emulation (four summation orders of the same network) differ from each other by less than 0.002 in the
    cosine median and 0.02 in the norm-ratio quantile (asserted below); the control has to miss the median bound by 0.01 and the norm-ratio
    bound by another 0.05 (the allowed margin once more) -- at least five and 2.5 times that noise."""
    y = tr.load_yardstick()
    assert y["sum_orders"] == list(tr.SUM_ORDERS)
    yard = y["cases"][key]
    shift = float(key.split("/")[1])
    assert [r["sum_order"] for r in yard["envelope"]] == list(tr.SUM_ORDERS) and yard["parameters"] > 200
    assert set(k.rsplit(".", 1)[1] for k in yard["running_err"]) == {"running_mean", "running_var"} and max(yard["running_err"].values()) < 5e-2
    for r in yard["envelope"]:
        assert tr.gradient_violations(r, yard, shift) == [], r
    medians, quantiles = [r["median"] for r in yard["envelope"]], [r["lr_q95"] for r in yard["envelope"]]
    assert max(medians) - min(medians) < 0.002 and max(quantiles) - min(quantiles) < 0.02
    control = yard["control_local_bn"]
    median_bound = max(yard["emulation"]["median"] - tr.MEDIAN_MARGIN, tr.FLOORS[shift][0])
    q05_bound = max(yard["emulation"]["q05"] - tr.Q05_MARGIN, tr.FLOORS[shift][1])
    assert control["median"] <= median_bound - 0.01, (control["median"], median_bound)
    assert control["q05"] <= q05_bound - 0.01, (control["q05"], q05_bound)
    assert control["lr_q95"] >= tr.log_ratio_bound(yard) + 0.05, (control["lr_q95"], tr.log_ratio_bound(yard))
    missed = tr.gradient_violations(control, yard, shift)
    assert any("cosine median" in m for m in missed) and any("norm ratio" in m for m in missed), missed
