"""Two real ranks with DIFFERENT data on one GPU (gloo, both on cuda:0): the host side of SyncBN in the backward, GradSync and the
evaluators' gathers -- everything ``engine.py`` / ``engine_bwd.py`` do around the collectives -- against the CPU oracle with autograd on
the CONCATENATED batch (tests/two_rank.py: launcher, cases, functional and bounds; tests/two_rank_worker.py: the ranks).

The ranks hold 3 + 1 sweeps (c32) / 1 + 1 (rv-av2 widths) and rank 1's sweeps are scaled and offset per channel, so that rank-local and global
statistics differ by O(1): the oracle run per rank slice with local BatchNorm (recorded in tests/golden/two_rank_yardstick.json and
asserted in tests/test_two_rank_cpu.py) and the two sabotaged device runs here land far outside the bounds the real runs are held to.

Bounds (tests/two_rank.py ``gradient_violations`` / ``running_violations``), g = sum over the ranks of the local ``p.grad``:
per-parameter cosine against the fp32 oracle -- median >= the CPU bf16 emulation's - 0.03, 5 % quantile >= its - 0.05, and the floors of
test_detector_gradients_vs_oracle; 95 % quantile of |log(|g| / |g32|)| <= the emulation's own over four summation orders (envelope
maximum) + 0.05 (a factor of two is 0.69); running statistics ``torch.equal`` across the ranks and within 1.5 x (emulation vs fp32)
+ 1e-3 of the oracle's.
"""

from __future__ import annotations

import pytest
import torch

import two_rank as tr

pytestmark = pytest.mark.gpu

# Time limit of every launch: three times the first clean run and at least 120 s.  First clean runs on an MI355X (two ranks, start of the
# processes to their exit): model c32, two shifts x four variants 3.8 s (one rank, one variant 2.4 s); either sabotaged run 2.8 - 3.0 s; model
# rv-av2 widths 3.4 s (one rank 3.5 s); gradsync 3.1 s; evaluator 3.9 s -- so the floor of 120 s is the limit everywhere.  (The wall time of
# these tests is the fp32 oracle on the CPU: about 5 s per c32 case and 25 s for the rv-av2 widths.)
LIMIT_S = 120.0

_ORACLE = {}


def _oracle(name, shift):
    """The fp32 oracle on the concatenated batch: computed once per session and shared, never modified."""
    key = tr.case_key(name, shift)
    if key not in _ORACLE:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        L32, g32, run32 = tr.oracle_run(tr.build_case(name, shift), tr.fp32_numerics())
        yard = tr.load_yardstick()["cases"][key]
        assert abs(L32 - yard["L32"]) <= 1e-4 * abs(yard["L32"]), (L32, yard["L32"])  # (the case the yardstick was recorded for)
        _ORACLE[key] = (L32, g32, run32, yard)
    return _ORACLE[key]


def _summed(results, run, what="grads"):
    """Sum over the ranks, on the CPU (a route of its own: torch adds what autograd accumulated per rank)."""
    out = {k: v.double().clone() for k, v in results[0]["runs"][run][what].items()}
    for r in results[1:]:
        for k, v in r["runs"][run][what].items():
            out[k] += v.double()
    return out


def _report(tag, m, yard):
    emu = yard["emulation"]
    print(f"    {tag}: {m['parameters']} parameters; cosine vs fp32 median {m['median']:.4f} q05 {m['q05']:.4f} min {m['min']:.4f} "
          f"(emulation {emu['median']:.4f} / {emu['q05']:.4f} / {emu['min']:.4f}); |log norm ratio| q95 {m['lr_q95']:.4f} max {m['lr_max']:.4f} "
          f"(emulation q95 {emu['lr_q95']:.4f}, bound {tr.log_ratio_bound(yard):.4f}); worst {m['worst'][0][0]} {m['worst'][0][1]:.4f}")


def _check_run(name, shift, results, variant, tag):
    """Every criterion of one (shift, variant) of a clean launch; returns the gradient metrics."""
    L32, g32, run32, yard = _oracle(name, shift)
    run = f"{shift}/{variant}"
    L = sum(r["runs"][run]["loss"] for r in results)
    m = tr.grad_metrics(_summed(results, run), g32)
    _report(f"{tag} shift {shift} {variant} (L {L:.5f}, fp32 {L32:.5f})", m, yard)
    assert tr.gradient_violations(m, yard, shift) == [], (tag, run)
    first = results[0]["runs"][run]["running"]
    for r in results[1:]:  # both ranks finalise from the same all-reduced totals
        for k, v in first.items():
            assert torch.equal(v, r["runs"][run]["running"][k]), (tag, run, k)
    assert all(int(v) == 1 for k, v in first.items() if k.endswith("num_batches_tracked"))
    worst = max(run32, key=lambda k: tr.rel_err(first[k].float(), run32[k]) / (1.5 * yard["running_err"][k] + 1e-3))
    print(f"        running statistics vs the fp32 oracle, nearest to its bound: {worst} {tr.rel_err(first[worst].float(), run32[worst]):.3e} "
          f"(emulation {yard['running_err'][worst]:.3e}; the emulation's largest {max(yard['running_err'].values()):.3e})")
    assert tr.running_violations(first, run32, yard) == [], (tag, run)
    return m


C32_CALLS = {"rv_reduce_rows_count", "rv_bn_bwd_reduce_pair", "rv_bn_bwd_apply_pair", "rv_bn_bwd_smallk_sums", "rv_bn_bwd_smallk_from_sums",
             "rv_bn_finalize", "rv_bn_bwd_finalize"}
VARIANTS = ("default", "no_group", "no_pair", "no_hold")


def test_c32_gradients_of_two_ranks_against_the_oracle_on_the_concatenated_batch(tmp_path):
    """3 + 1 heterogeneous sweeps, BatchNorm shifts 6.0 and 3.0, four variants of the host-side routes in one launch; the one-rank run on all
    four sweeps beside it as a diagnostic held to the same bounds (not the reference)."""
    (tmp_path / "two").mkdir()
    (tmp_path / "one").mkdir()
    two = tr.launch("model", 2, tmp_path / "two", ["--case", "c32", "--shifts", "6.0,3.0", "--variants", ",".join(VARIANTS)], limit_s=LIMIT_S)
    one = tr.launch("model", 1, tmp_path / "one", ["--case", "c32", "--shifts", "6.0,3.0", "--variants", "default"], limit_s=LIMIT_S)
    for shift in (6.0, 3.0):
        _check_run("c32", shift, one, "default", "one rank")
        for variant in VARIANTS:
            _check_run("c32", shift, two, variant, "two ranks")
            a, b = two[0]["runs"][f"{shift}/{variant}"], two[1]["runs"][f"{shift}/{variant}"]
            assert a["collectives"] == b["collectives"] > 100, (variant, a["collectives"], b["collectives"])
        runs = {v: two[0]["runs"][f"{shift}/{v}"] for v in VARIANTS}
        calls = set(runs["default"]["calls"])
        assert C32_CALLS <= calls, sorted(C32_CALLS - calls)
        print(f"    shift {shift}: collectives per step {[(v, runs[v]['collectives']) for v in VARIANTS]}; "
              f"rv_head_final_bwd_apply taken: {'rv_head_final_bwd_apply' in calls}")
        # the switches switch: ungrouped layers pay one collective each, and without the pair form the one-pass pair kernels are gone
        assert runs["no_group"]["collectives"] > runs["default"]["collectives"] == runs["no_hold"]["collectives"]
        assert not {"rv_bn_bwd_reduce_pair", "rv_bn_bwd_apply_pair"} & set(runs["no_pair"]["calls"])
        assert "rv_bn_bwd_reduce_pair" in runs["no_group"]["calls"] and "rv_bn_bwd_apply_pair" not in runs["no_group"]["calls"]
        assert one[0]["runs"][f"{shift}/default"]["collectives"] == 0 and "rv_reduce_rows_count" not in one[0]["runs"][f"{shift}/default"]["calls"]


@pytest.mark.parametrize("sabotage", ["backward_local", "forward_local"])
def test_c32_a_rank_local_syncbn_is_outside_the_bounds(tmp_path, sabotage):
    """Negative control on the device: ``engine.all_reduce_`` is the identity during the backward, resp. the forward (both ranks skip
    consistently: wrong numbers, nothing else) -- the criteria of the test above must be VIOLATED."""
    two = tr.launch("model", 2, tmp_path, ["--case", "c32", "--shifts", "6.0,3.0", "--variants", "default", "--sabotage", sabotage], limit_s=LIMIT_S)
    for shift in (6.0, 3.0):
        _, g32, run32, yard = _oracle("c32", shift)
        run = f"{shift}/default"
        m = tr.grad_metrics(_summed(two, run), g32)
        _report(f"{sabotage} shift {shift}", m, yard)
        broken = tr.gradient_violations(m, yard, shift)
        print("    violated:", broken)
        assert broken, (sabotage, shift, m)
        if sabotage == "forward_local":  # each rank finalised from its own totals: the running statistics differ and miss the oracle's
            a, b = two[0]["runs"][run]["running"], two[1]["runs"][run]["running"]
            assert any(not torch.equal(a[k], b[k]) for k in a)
            assert tr.running_violations(a, run32, yard) and tr.running_violations(b, run32, yard)


REAL_WIDTH_CALLS = {"rv_reduce_rows_count", "rv_pos_forward", "rv_pos_backward_sums", "rv_meta_modulate_bwd_sums", "rv_meta_modulate_bwd_apply",
                    "rv_head_final_bwd_sums", "rv_head_final_bwd_apply", "rv_bn_finalize", "rv_bn_bwd_finalize", "rv_bn_bwd_smallk_from_sums"}


def test_rv_av2_widths_gradients_of_two_ranks_against_the_oracle(tmp_path):
    """The benchmarked widths (256-channel positional pair, 512-channel towers) on 1 + 1 heterogeneous sweeps of 64 x 256, shift 3.0."""
    (tmp_path / "two").mkdir()
    (tmp_path / "one").mkdir()
    two = tr.launch("model", 2, tmp_path / "two", ["--case", "rv-av2", "--shifts", "3.0", "--variants", "default"], limit_s=LIMIT_S)
    one = tr.launch("model", 1, tmp_path / "one", ["--case", "rv-av2", "--shifts", "3.0", "--variants", "default"], limit_s=LIMIT_S)
    _check_run("rv-av2", 3.0, one, "default", "one rank")
    _check_run("rv-av2", 3.0, two, "default", "two ranks")
    a, b = two[0]["runs"]["3.0/default"], two[1]["runs"]["3.0/default"]
    assert a["collectives"] == b["collectives"] > 100, (a["collectives"], b["collectives"])
    assert REAL_WIDTH_CALLS <= set(a["calls"]), sorted(REAL_WIDTH_CALLS - set(a["calls"]))
    kernels = a["kernels"]
    assert "wgrad3_kernel(+reduce)" in kernels and any(k.startswith(("tapconv5_kernel<", "tapconv6_kernel<")) for k in kernels), kernels


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_grad_sync_with_two_real_ranks(tmp_path):
    """``engine.GradSync`` (flat buffer, one all-reduce per run of a node's parameters, one scaling) against an independent route: autograd's own
    accumulation per rank and a torch sum.  One-task head and a two-task head whose nodes' parameters are not contiguous in the flat buffer; two
    steps."""
    two = tr.launch("gradsync", 2, tmp_path, ["--shifts", "6.0"], limit_s=LIMIT_S)
    for kind in ("one_task", "two_tasks"):
        a, b = two[0]["runs"][kind], two[1]["runs"][kind]
        # run-to-run difference of the plain route (the same step twice on each rank), per parameter, relative L2
        repeat = max(_rel_l2(r["plain2"][k], r["plain1"][k]) for r in (a, b) for k in r["plain1"])
        bitwise = all(torch.equal(r["plain2"][k], r["plain1"][k]) for r in (a, b) for k in r["plain1"])
        # bound: 1e-6 where the plain route repeats bit for bit, else twice its measured run-to-run difference.  Measured on an MI355X: the
        # plain route repeats bit for bit on both ranks with either head (run-to-run difference 0.0), so the bound in force is 1e-6; the
        # worst parameter then measures 4.3e-8 (the fp32 rounding of the all-reduce's one addition against the float64 sum taken here)
        bound = 1e-6 if bitwise else 2.0 * repeat
        worst = 0.0
        for step in ("sync1", "sync2"):
            for k, v in a[step].items():
                assert torch.equal(v, b[step][k]), (kind, step, k)  # the same averaged gradient on both ranks
                want = a["plain1"][k].double() + b["plain1"][k].double()
                err = _rel_l2(2.0 * v.double(), want)
                worst = max(worst, err)
                assert err <= bound, (kind, step, k, err, bound)
        print(f"    gradsync {kind}: plain route run-to-run {repeat:.3e} (bit for bit: {bitwise}), bound {bound:.3e}, world * p.grad vs the summed plain "
              f"gradients: worst {worst:.3e}; all-reduce runs per node {a['node_runs']}")
        assert a["node_runs"] == b["node_runs"]
        if kind == "two_tasks":  # a task's towers are cut into more than one run of the flat buffer
            assert max(a["node_runs"]) >= 2, a["node_runs"]
        else:  # the one-task run against the oracle, with the bounds of the model-level test
            _, g32, _, yard = _oracle("c32", 6.0)
            m = tr.grad_metrics({k: 2.0 * v for k, v in a["sync1"].items()}, g32)
            _report("gradsync one task, world * p.grad", m, yard)
            assert tr.gradient_violations(m, yard, 6.0) == []


def test_evaluators_over_two_ranks(tmp_path):
    """Three sweeps; split A: rank 0 holds sweeps {0, 1}, rank 1 {2} (unequal row counts); split B: rank 1 holds ground truth but no
    detection (zero rows).  ``compute()`` on EACH rank equals, exactly, the table of one evaluator that saw all three sweeps in one process --
    ``DetectionEvaluator`` (sizes gathered, rows padded, counts summed) and ``WaymoDetectionEvaluator`` (integer tables all-reduced)."""
    two = tr.launch("evaluator", 2, tmp_path, limit_s=LIMIT_S)
    for split in ("A", "B"):
        a, b = two[0]["splits"][split], two[1]["splits"][split]
        print(f"    split {split}: detection rows {a['rows']} + {b['rows']} (Waymo {a['waymo_rows']} + {b['waymo_rows']}); AP {a['ap']:.4f}, n_dts {a['n_dts']}, "
              f"n_gts {a['n_gts']}; Waymo counted {a['waymo_counts']}, best value {a['waymo_max']:.4f}")
        assert a["rows"] > b["rows"] and (b["rows"] == 0) == (split == "B") and (b["waymo_rows"] == 0) == (split == "B")
        for r in (a, b):
            assert r["av2_equal"], (split, r["av2"], r["av2_want"])
            assert r["waymo_tables_equal"] and r["waymo_equal"], split
            assert r["n_dts"] > 100 and r["n_gts"] > 50 and 0.0 < r["ap"] < 1.0 and r["waymo_counts"] > 100 and r["waymo_max"] > 0.05  # (not vacuous)
