"""Yardstick of the full-size GPU tests: what bf16 storage costs the CPU EMULATION of the model (oracle, ``Numerics.bf16``) against
the fp32 oracle, at the benchmarked widths and image sizes.  The crop tests (tests/test_gpu_realwidth.py) compute this yardstick
on the fly; at 64 x 2048 / 64 x 2656 one emulation pass costs 50-80 s of a 16-core host per test, so it is measured ONCE with this
script and recorded in tests/test_gpu_fullsize_train.py (``EMULATION``).  CPU only; run from the repo root:

    python tests/tools/emulation_yardstick.py [rv-av2|rv-waymo|base-av2|base-waymo|first-step]
    python tests/tools/emulation_yardstick.py envelope [case key ...]   # rewrites tests/golden/emulation_envelope.json (given keys: only those cases)
    python tests/tools/emulation_yardstick.py two-rank [case key ...]   # rewrites tests/golden/two_rank_yardstick.json (see ``two_rank``)

``envelope`` (round-5 review, item 9): the crop cases of tests/test_gpu_realwidth.py under EIGHT summation orders of the CPU bf16
emulation (``Numerics.bf16(sum_order=k)``: every conv visits its input channels in a permuted order -- the same network, another
valid fp32 rounding of every accumulation).  In the chaotic regime (BatchNorm shifts around zero: half of the ReLU gates within a
bf16 ulp of zero) two such realisations differ from each other as much as each differs from fp32; min / max of the per-parameter
gradient cosine's median and 5 % quantile over the realisations is the ENVELOPE the HIP result is asserted against (envelope minimum
- 0.02), instead of a margin that was re-tuned whenever a kernel changed.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def train_case(widths, n_feat, n_cls, W):
    from oracle import model as om
    from oracle import targets as otgt
    from test_gpu_realwidth import _prepare, stem_type_of

    _, _, sd, batch = _prepare(widths, n_feat, n_cls, W, 3.0)

    def run(nm):
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
        _, logits, reg = om.detector_forward(batch["features"], batch["cart"], {**sd, **params}, stem_type=stem_type_of(widths), nm=nm)
        tg = otgt.compute_targets(batch["cart"], batch["annotations"], n_cls)
        loss = otgt.detection_loss(logits, reg, batch["cart"], batch["mask"], tg, n_cls)["loss"]
        loss.backward()
        return logits.detach(), reg.detach(), float(loss.detach()), {k: p.grad for k, p in params.items()}

    lg32, rg32, loss32, g32 = run(om.Numerics(train=True))
    lg16, rg16, loss16, g16 = run(om.Numerics.bf16(train=True))
    cos = np.array([_cos(g16[k], g32[k]) for k in g32 if float(g32[k].norm()) >= 1e-9])
    return {"emu~fp32": rel_err(lg16, lg32), "reg emu~fp32": rel_err(rg16, rg32), "cos_logits": _cos(lg16, lg32), "cos_reg": _cos(rg16, rg32),
            "loss32": loss32, "loss16": loss16, "grad_cos_median": float(np.median(cos)), "grad_cos_q05": float(np.quantile(cos, 0.05)),
            "grad_cos_min": float(cos.min()), "threads": torch.get_num_threads()}


def first_step():
    import bench
    from oracle import model as om
    from oracle import targets as otgt

    torch.manual_seed(0)
    backbone, head = bench.build_model("rv-av2", bench.AV2_CLASSES)
    sd = {**{f"backbone.{k}": v for k, v in backbone.state_dict().items()}, **{f"head.{k}": v for k, v in head.state_dict().items()}}
    batch = bench.synthetic_batch(1, 64, 2048, seed=1234, device="cpu")
    tg = otgt.compute_targets(batch["cart"], batch["annotations"], bench.AV2_CLASSES)
    out = {}
    with torch.no_grad():
        for name, nm in (("loss32", om.Numerics(train=True)), ("loss16", om.Numerics.bf16(train=True))):
            _, logits, reg = om.detector_forward(batch["features"], batch["cart"], sd, nm=nm)
            out[name] = float(otgt.detection_loss(logits, reg, batch["cart"], batch["mask"], tg, bench.AV2_CLASSES)["loss"])
    return out


ENVELOPE_CASES = {"rv-av2/256/3.0": ("rv-av2", 5, 26, 256, 3.0), "rv-av2/256/0.0": ("rv-av2", 5, 26, 256, 0.0), "rv-waymo/336/3.0": ("rv-waymo", 6, 3, 336, 3.0),
                  "base-av2/256/3.0": ("base-av2", 5, 26, 256, 3.0), "base-av2/256/0.0": ("base-av2", 5, 26, 256, 0.0),
                  "base-waymo/336/3.0": ("base-waymo", 6, 3, 336, 3.0)}
ENVELOPE_ORDERS = (0, 1, 2, 3, 4, 5, 6, 7)


def envelope_case(widths, n_feat, n_cls, W, shift):
    from oracle import model as om
    from oracle import targets as otgt
    from test_gpu_realwidth import _prepare, stem_type_of

    _, _, sd, batch = _prepare(widths, n_feat, n_cls, W, shift)

    def run(nm):
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k}
        _, logits, reg = om.detector_forward(batch["features"], batch["cart"], {**sd, **params}, stem_type=stem_type_of(widths), nm=nm)
        tg = otgt.compute_targets(batch["cart"], batch["annotations"], n_cls)
        loss = otgt.detection_loss(logits, reg, batch["cart"], batch["mask"], tg, n_cls)["loss"]
        loss.backward()
        return float(loss.detach()), {k: p.grad for k, p in params.items()}

    loss32, g32 = run(om.Numerics(train=True))
    keys = [k for k in g32 if float(g32[k].norm()) >= 1e-9]
    # the permuted order is the same network: in fp32 its gradients agree with the stored order to fp32 rounding
    _, g32p = run(om.Numerics(train=True, sum_order=2))
    fp32_check = min(_cos(g32p[k], g32[k]) for k in keys)
    rows = []
    for order in ENVELOPE_ORDERS:
        loss16, g16 = run(om.Numerics.bf16(train=True, sum_order=order))
        cos = np.array([_cos(g16[k], g32[k]) for k in keys])
        rows.append({"sum_order": order, "loss16": loss16, "median": float(np.median(cos)), "q05": float(np.quantile(cos, 0.05)), "min": float(cos.min())})
        print("   ", rows[-1], flush=True)
    return {"loss32": loss32, "parameters": len(keys), "fp32_permuted_order_min_cos": fp32_check, "realisations": rows,
            "median_min": min(r["median"] for r in rows), "median_max": max(r["median"] for r in rows),
            "q05_min": min(r["q05"] for r in rows), "q05_max": max(r["q05"] for r in rows)}


def two_rank(wanted):
    """tests/golden/two_rank_yardstick.json: the CPU side of tests/test_gpu_two_rank.py (cases, functional and arithmetic in
    tests/two_rank.py) -- per case the fp32 oracle's functional value, the bf16 emulation's per-parameter gradient cosine and
    |log norm ratio| against fp32 under four summation orders, its running statistics' distance from fp32, and the local-BatchNorm
    control (the oracle per rank slice, gradients summed): what a rank-local SyncBN would score."""
    import two_rank as tr

    out = {}
    if wanted and os.path.exists(tr.YARDSTICK):
        out = tr.load_yardstick()["cases"]
    for name, spec in tr.CASES.items():
        for shift in spec[6]:
            key = tr.case_key(name, shift)
            if wanted and key not in wanted:
                continue
            print(key, flush=True)
            out[key] = tr.record_case(name, shift)
    with open(tr.YARDSTICK, "w") as f:
        json.dump({"threads": torch.get_num_threads(), "torch": torch.__version__, "sum_orders": list(tr.SUM_ORDERS), "cases": out}, f, indent=1)
        f.write("\n")
    print("wrote", tr.YARDSTICK)


if __name__ == "__main__":
    if sys.argv[1:2] == ["two-rank"]:
        two_rank(sys.argv[2:])
        sys.exit(0)
    if sys.argv[1:2] == ["envelope"]:
        path = os.path.join(ROOT, "tests", "golden", "emulation_envelope.json")
        wanted = sys.argv[2:]  # case keys to (re-)record; the other cases keep their recorded values
        out = {}
        if wanted:
            with open(path) as f:
                out = json.load(f)["cases"]
        for name, case in ENVELOPE_CASES.items():
            if wanted and name not in wanted:
                continue
            print(name, flush=True)
            out[name] = envelope_case(*case)
        with open(path, "w") as f:
            json.dump({"threads": torch.get_num_threads(), "torch": torch.__version__, "cases": out}, f, indent=1)
            f.write("\n")
        print("wrote", path)
        sys.exit(0)
    which = sys.argv[1:] or ["rv-av2", "rv-waymo", "base-av2", "base-waymo", "first-step"]
    for w in which:
        r = first_step() if w == "first-step" else train_case(*{"rv-av2": ("rv-av2", 5, 26, 2048), "rv-waymo": ("rv-waymo", 6, 3, 2656),
                                                                     "base-av2": ("base-av2", 5, 26, 2048), "base-waymo": ("base-waymo", 6, 3, 2656)}[w])
        print(w, json.dumps(r), flush=True)
