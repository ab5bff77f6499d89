"""One rank of a tests/two_rank.py launch.  Options come from ``argv``; the result goes to ``<dir>/rank<r>.pt`` (CPU tensors and plain
values).  Modes:

``cpu``        launcher checks, no GPU: an all-reduce round trip; ``--fail-rank R`` lets rank R exit with status 3 instead of entering
               the collective its peer waits in.
``model``      the composed model on this rank's slice of a tests/two_rank.py case under SyncBN, the linear functional, backward:
               local ``p.grad`` (no GradSync), running statistics, the census of library calls and collectives, per variant of the
               host-side routes.  ``--sabotage backward_local | forward_local``: ``engine.all_reduce_`` is the identity while the backward /
               the forward runs (both ranks skip consistently: wrong numbers, nothing waits).
``gradsync``   ``engine.GradSync`` against autograd's own accumulation, two steps, one-task and two-task head.
``evaluator``  ``DetectionEvaluator`` / ``WaymoDetectionEvaluator`` over unequal row counts and a rank without detections, against one
               evaluator that saw every sweep in this process (computed before the process group exists).

Every module attribute the worker changes (``engine.SYNC_BN``, ``engine.GRAD_SYNC``, the route switches, the call spy) is put back.
"""

from __future__ import annotations

import argparse
import datetime
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda:0"


def _init(args, device: bool = True) -> None:
    if device:
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(args.dir, 'rendezvous')}", rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=args.collective_timeout))


def _save(args, result: dict) -> None:
    path = os.path.join(args.dir, f"rank{args.rank}.pt")
    torch.save(result, path + ".tmp")
    os.replace(path + ".tmp", path)


# ------------------------------------------------------------------------------------------------------------------------------------
def mode_cpu(args) -> dict:
    _init(args, device=False)
    if args.fail_rank == args.rank:
        print(f"rank {args.rank}: leaving with status 3 before the collective", flush=True)
        os._exit(3)
    t = torch.arange(4, dtype=torch.float64) + 10.0 * args.rank
    dist.all_reduce(t)
    return {"rank": args.rank, "sum": t}


# ------------------------------------------------------------------------------------------------------------------------------------
class _Census:
    """Names of the library calls issued inside the block (the pattern of tests/test_gpu_optim_groups.py)."""

    def __enter__(self):
        from range_view_3d_detection_amd import _lib as L

        self.names, self.real = set(), L._call

        def spy(name, *a):
            self.names.add(name)
            return self.real(name, *a)

        L._call = spy
        return self.names

    def __exit__(self, *exc):
        from range_view_3d_detection_amd import _lib as L

        L._call = self.real


class _Switches:
    """Route switches of one variant, and SyncBN on for more than one rank; everything back on exit."""

    VARIANTS = {"default": {}, "no_group": {"GROUP_SYNC_BN": False}, "no_pair": {"BNB_PAIR": False}, "no_hold": {"HOLD_WGRAD_FOR_SYNC_BN": False}}

    def __init__(self, variant: str, world: int) -> None:
        self.set, self.world = self.VARIANTS[variant], world

    def __enter__(self):
        from range_view_3d_detection_amd import engine as E
        from range_view_3d_detection_amd import engine_bwd

        self.saved = [(E, "SYNC_BN", E.SYNC_BN), (E, "GROUP_SYNC_BN", E.GROUP_SYNC_BN), (engine_bwd, "BNB_PAIR", engine_bwd.BNB_PAIR),
                      (E, "HOLD_WGRAD_FOR_SYNC_BN", E.HOLD_WGRAD_FOR_SYNC_BN), (E, "PROFILE", E.PROFILE), (E, "GRAD_SYNC", E.GRAD_SYNC)]
        if self.world > 1:
            E.SYNC_BN = True
        for k, v in self.set.items():
            setattr(engine_bwd if k == "BNB_PAIR" else E, k, v)
        return self

    def __exit__(self, *exc):
        for mod, k, v in self.saved:
            setattr(mod, k, v)


class _LocalAllReduce:
    """``engine.all_reduce_`` as the identity inside the block (the negative controls)."""

    def __init__(self, on: bool) -> None:
        self.on = on

    def __enter__(self):
        from range_view_3d_detection_amd import engine as E

        self.real = E.all_reduce_
        if self.on:
            E.all_reduce_ = lambda t: None

    def __exit__(self, *exc):
        from range_view_3d_detection_amd import engine as E

        E.all_reduce_ = self.real


def _rank_data(case: dict, name: str, args):
    import two_rank as tr

    lo, hi = tr.rank_slices(name, args.world)[args.rank]
    data = {"features": case["features"][lo:hi].to(DEV), "cart": case["cart"][lo:hi].to(DEV), "mask": case["mask"][lo:hi].to(DEV)}
    return data, case["Rl"][lo:hi].to(DEV), case["Rr"][lo:hi].to(DEV)


def _step(model, data, Rl, Rr, pixels: int, sabotage: str = "none", tasks=(0,)):
    """Forward in training mode, the functional over every task's outputs, backward.  ``Rl`` holds the tasks' classes back to back."""
    import two_rank as tr

    with _LocalAllReduce(sabotage == "forward_local"):
        feats = model.backbone(data)
        outputs, _ = model.head(feats, data, return_loss=False)
        loss, c0 = 0.0, 0
        for t in tasks:
            logits, reg = outputs[1][t]["logits"], outputs[1][t]["regressands"]
            n = logits.shape[1]
            loss = loss + tr.functional(logits, reg, Rl[:, c0:c0 + n], Rr, pixels)
            c0 += n
    with _LocalAllReduce(sabotage == "backward_local"):
        loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach())


def _grads(model) -> dict:
    return {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters()}


def mode_model(args) -> dict:
    import bench
    import two_rank as tr
    from range_view_3d_detection_amd import engine as E

    _init(args)
    real_width = args.case != "c32"
    if real_width:
        from test_gpu_realwidth import _small_grids  # (crops: lift the tile-count heuristic so that the production kernels run)
    runs = {}
    for shift in [float(s) for s in args.shifts.split(",")]:
        for variant in args.variants.split(","):
            case = tr.build_case(args.case, shift)
            model = bench.Detector(case["backbone"], case["head"]).to(DEV).train()
            data, Rl, Rr = _rank_data(case, args.case, args)
            E.COLLECTIVES.reset()
            with _Switches(variant, args.world), _Census() as names:
                if real_width:
                    E.PROFILE = E.KernelProfile()
                    with _small_grids(True):
                        loss = _step(model, data, Rl, Rr, case["pixels"], args.sabotage)
                    kernels = sorted(set(name for name, *_ in E.PROFILE.records))
                else:
                    loss, kernels = _step(model, data, Rl, Rr, case["pixels"], args.sabotage), []
            running = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
            runs[f"{shift}/{variant}"] = {"loss": loss, "grads": _grads(model), "running": running, "calls": sorted(names), "kernels": kernels,
                                         "collectives": E.COLLECTIVES.calls}
            print(f"rank {args.rank}: {args.case} shift {shift} {variant}: L {loss:.6f}, {E.COLLECTIVES.calls} collectives", flush=True)
            del model, case
    assert E.SYNC_BN is None and E.GRAD_SYNC is None and E.PROFILE is None
    return {"rank": args.rank, "runs": runs}


# ------------------------------------------------------------------------------------------------------------------------------------
TWO_TASKS = {0: ["C0", "C1", "C2"], 1: ["D0", "D1"]}


def _two_task_head(head):
    """The c32 head of bench.build_model with two tasks on its one level: the towers of a task (one autograd node) are not contiguous in
    ``head.parameters()`` -- every classification tower is registered before the regression towers."""
    from range_view_3d_detection_amd.nn.heads.detection_head import DetectionHead

    tcfg = dict(head.targets_config, tasks=TWO_TASKS)
    return DetectionHead(fpn=head.fpn, fpn_kernel_sizes=head.fpn_kernel_sizes, targets_config=tcfg, num_classification_blocks=head.num_classification_blocks,
                         num_regression_blocks=head.num_regression_blocks, final_kernel_size=head.final_kernel_size, tasks_cfg=TWO_TASKS,
                         task_in_channels=head.task_in_channels, classification_weight=1.0, regression_weight=1.0, coding_weights=[1.0] * 8,
                         classification_head_channels=head.classification_head_channels, regression_head_channels=head.regression_head_channels,
                         classification_normalization_method="FOREGROUND",
                         _cls_loss={"_target_": "torchbox3d.nn.losses.classification.VarifocalLoss", "alpha": 0.75, "gamma": 2.0, "reduction": "none"},
                         _regression_loss={"_target_": "torch.nn.L1Loss", "reduction": "none"})


def mode_gradsync(args) -> dict:
    import bench
    import two_rank as tr
    from range_view_3d_detection_amd import engine as E

    _init(args)
    shift = float(args.shifts.split(",")[0])
    runs = {}
    for kind in ("one_task", "two_tasks"):
        case = tr.build_case("c32", shift)
        head, tasks = case["head"], (0,)
        if kind == "two_tasks":
            torch.manual_seed(2)
            head, tasks = _two_task_head(case["head"]), (0, 1)
            gen = torch.Generator().manual_seed(3)
            for m in head.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=gen)
                    m.bias.data = 0.2 * torch.randn(m.bias.shape, generator=gen) + shift
        model = bench.Detector(case["backbone"], head).to(DEV).train()
        data, Rl, Rr = _rank_data(case, "c32", args)
        params = [p for p in model.parameters() if p.requires_grad]
        out = {}
        with _Switches("default", args.world):
            for tag in ("plain1", "plain2"):  # autograd's own accumulation, twice: the run-to-run difference sizes the bound
                model.zero_grad(set_to_none=True)
                _step(model, data, Rl, Rr, case["pixels"], tasks=tasks)
                out[tag] = _grads(model)
            gs = E.GradSync(params, args.world)
            node_runs, real_reduce = [], gs.reduce_node

            def counted(ps, gr):
                before = len(gs.works)
                res = real_reduce(ps, gr)
                node_runs.append(len(gs.works) - before)
                return res

            gs.reduce_node = counted
            E.GRAD_SYNC = gs
            for tag in ("sync1", "sync2"):  # the second step after zero_grad(set_to_none=True)
                model.zero_grad(set_to_none=True)
                _step(model, data, Rl, Rr, case["pixels"], tasks=tasks)
                gs.finish()
                torch.cuda.synchronize()
                out[tag] = _grads(model)
        out["node_runs"] = node_runs
        runs[kind] = out
        print(f"rank {args.rank}: gradsync {kind}: all-reduce runs per node {node_runs}", flush=True)
    assert E.SYNC_BN is None and E.GRAD_SYNC is None
    return {"rank": args.rank, "runs": runs}


# ------------------------------------------------------------------------------------------------------------------------------------
def _table_cols(table) -> dict:
    return {c: table.column(c).to_pylist() for c in table.column_names}


def mode_evaluator(args) -> dict:
    import numpy as np

    torch.cuda.set_device(0)
    import test_gpu_evaluation as te
    import test_gpu_waymo_evaluation as tw
    import waymo_eval_ref as wref
    from range_view_3d_detection_amd.evaluation import DetectionEvaluator, WaymoDetectionEvaluator
    from test_evaluation_cpu import _cfg

    n_cat, names = 5, [f"C{i}" for i in range(5)]
    cfg = _cfg(n_cat)
    g = np.random.default_rng(20261020)
    av2 = te._scene(g, 3, n_cat, max_gt=20, max_dt=200)
    by_sweep = np.argsort(av2["dt_sweep"], kind="stable")  # rows grouped by sweep: the gathered order is the one-process order
    for k in ("dts", "scores", "dt_sweep", "dt_cat"):
        av2[k] = av2[k][by_sweep]
    wm = tw._crowded_scene(g, 3, (1, 2, 200, 40))
    by_sweep = np.argsort(wm["dt_sweep"], kind="stable")
    for k in ("dts", "scores", "dt_sweep", "dt_type"):
        wm[k] = wm[k][by_sweep]
    wm["dt_rows"], wm["gt_rows"] = wref.rows_from_yaw(wm["dts"]), wref.rows_from_yaw(wm["gts"])
    wm["gt_npts"] = np.where(wm["gt_level"] == 0, 0, np.where(wm["gt_level"] == 2, 3, 50))
    wm["gt_difficulty"] = np.zeros_like(wm["gt_npts"])

    def without_detections_of(scene, sweep, keys):
        keep = scene["dt_sweep"] != sweep
        return {k: (v[keep] if k in keys else v) for k, v in scene.items()}

    scenes = {"A": (av2, wm),  # rank 0: sweeps {0, 1}, rank 1: sweep {2} -- unequal row counts
              "B": (without_detections_of(av2, 2, ("dts", "scores", "dt_sweep", "dt_cat")),  # rank 1: ground truth, no detection
                    without_detections_of(wm, 2, ("dts", "dt_rows", "scores", "dt_sweep", "dt_type")))}
    mine = [[0, 1, 2]] if args.world == 1 else [[0, 1], [2]]

    def av2_evaluator(scene, sweeps):
        ev = DetectionEvaluator(cfg, names, max_sweeps=3)
        ann = np.zeros((len(scene["gts"]), 13))
        ann[:, :10], ann[:, 11], ann[:, 12] = scene["gts"], scene["gt_cat"], scene["gt_sweep"]
        d, a = np.isin(scene["dt_sweep"], sweeps), np.isin(scene["gt_sweep"], sweeps)
        ev.update(te._dev(scene["dts"][d]), te._dev(scene["scores"][d]), te._dev(scene["dt_cat"][d], torch.float32), te._dev(scene["dt_sweep"][d], torch.float32),
                  te._dev(ann[a]), num_interior_pts=te._dev(scene["gt_valid"][a]))
        return ev, int(d.sum())

    def waymo_evaluator(scene, sweeps):
        ev = WaymoDetectionEvaluator(idx_to_category=tw.NAMES, max_sweeps=3)
        ann = np.zeros((len(scene["gt_rows"]), 13))
        ann[:, :10], ann[:, 11], ann[:, 12] = scene["gt_rows"], scene["gt_type"] - 1, scene["gt_sweep"]
        d, a = np.isin(scene["dt_sweep"], sweeps), np.isin(scene["gt_sweep"], sweeps)
        ev.update(te._dev(scene["dt_rows"][d]), te._dev(scene["scores"][d]), te._dev(scene["dt_type"][d] - 1, torch.float32),
                  te._dev(scene["dt_sweep"][d], torch.float32), te._dev(ann[a]), te._dev(scene["gt_npts"][a]), te._dev(scene["gt_difficulty"][a]))
        return ev, int(d.sum())

    # one evaluator that saw all three sweeps in this process: no process group yet, so compute() gathers nothing
    assert not dist.is_initialized()
    want = {}
    for split, (s_av2, s_wm) in scenes.items():
        ev, _ = av2_evaluator(s_av2, [0, 1, 2])
        wev, _ = waymo_evaluator(s_wm, [0, 1, 2])
        want[split] = (ev.compute(), wev.tables().cpu(), wev.compute())
    _init(args)
    out = {}
    for split, (s_av2, s_wm) in scenes.items():
        ev, n_rows = av2_evaluator(s_av2, mine[args.rank])
        wev, n_wrows = waymo_evaluator(s_wm, mine[args.rank])
        table, counts, wtable = ev.compute(), wev.tables().cpu(), wev.compute()
        t_want, c_want, w_want = want[split]
        out[split] = {"av2_equal": bool(table.equals(t_want)), "waymo_tables_equal": bool(torch.equal(counts, c_want)), "waymo_equal": bool(wtable.equals(w_want)),
                      "rows": n_rows, "waymo_rows": n_wrows, "av2": _table_cols(table), "av2_want": _table_cols(t_want),
                      "n_dts": int(table.column("n_dts")[-1].as_py()), "n_gts": int(table.column("n_gts")[-1].as_py()),
                      "ap": float(table.column("AP")[-1].as_py()), "waymo_counts": int(counts[..., 0].sum()), "waymo_max": float(max(wtable.column("value").to_pylist()))}
        print(f"rank {args.rank}: evaluator split {split}: {n_rows} / {n_wrows} detection rows here; equal {out[split]['av2_equal']} "
              f"{out[split]['waymo_tables_equal']} {out[split]['waymo_equal']}", flush=True)
    return {"rank": args.rank, "splits": out}


# ------------------------------------------------------------------------------------------------------------------------------------
def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("cpu", "model", "gradsync", "evaluator"))
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--dir", required=True)
    ap.add_argument("--collective-timeout", type=float, default=60.0)
    ap.add_argument("--fail-rank", type=int, default=-1)
    ap.add_argument("--case", default="c32")
    ap.add_argument("--shifts", default="6.0")
    ap.add_argument("--variants", default="default")
    ap.add_argument("--sabotage", default="none", choices=("none", "backward_local", "forward_local"))
    args = ap.parse_args()
    result = {"cpu": mode_cpu, "model": mode_model, "gradsync": mode_gradsync, "evaluator": mode_evaluator}[args.mode](args)
    _save(args, result)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
