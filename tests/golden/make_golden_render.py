"""Fixtures for the debug panels: ``tests/golden/render/{functions,panels}.npz``.

Runs the REFERENCE's own ``normalize_apply_colormap``, ``build_bev`` and ``world_to_image`` (``rendering/tensorboard.py:187-211,
444-454``) and its ``draw_detections`` (``:253-441``) on the CPU, over ``make_golden``'s stubs plus the stand-ins added HERE for what
``rendering/tensorboard.py`` imports and this machine lacks:

* ``kornia.enhance.normalize.normalize_min_max``: ``(x - min) / (max - min + 1e-6)`` per channel (kornia's formula, eps 1e-6);
* ``cv2``: ``polylines`` / ``rectangle`` / ``putText`` are NO-OPS that hand the image back, so the fixtures hold no footprint and no
  text label -- they pin the panel order, both padding branches, the stacking and the point splat, not the (declared) line raster;
* ``torchvision.io.image.write_png``, ``matplotlib.cm.get_cmap`` (gone from matplotlib 3.9 on: ``matplotlib.colormaps[name]``),
  the Lightning names the module imports, polars' ``top_k``;
* ``mmcv.ops.boxes_iou3d``: the float64 clip of ``tests/waymo_eval_ref.py`` (its result only picks a colour for the no-op draw);
* ``Tensor.cuda`` (``:300,306``) is bound to the identity while ``draw_detections`` runs, so the frames WITH detections go through.

``functions.npz``: planes (random, constant, all-masked, single-pixel maximum) through ``normalize_apply_colormap`` with each of the
three colour tables (the tables themselves are stored too), point sets through ``build_bev`` and ``world_to_image``.
``panels.npz``: ``wide`` -- two samples, two levels (W 64 and 32 against a 40-pixel view: the view is padded at level 1, the panels at
level 2), two tasks, aux maps; ``narrow`` -- W 37 against the 40-pixel view (odd difference: left 1, right 2), one level, one task, no
aux.  ``max_side = 3.0``, ``meter_per_px = 0.15``.

Inputs are drawn in float64 and rounded to a grid that is exact in fp32.  A pixel whose point would land within 1e-3 px of a pixel
boundary, or whose normalised value times 255 lies within 1e-3 of an integer, takes the source values of a pixel that does not
(exact hits are kept: the plane's minimum maps to exactly 0; the maximum of a likelihood plane is checked to sit clear of the next
integer by 1e-4, a thousand fp32 ulps; the norm and abs planes are IEEE operations only, the same bit for bit everywhere), and the
generator asserts that none is left.  So nothing depends on whether a host divides or multiplies by a reciprocal, or on the last bits
of ``expf``.
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stubs and imports the reference)
import _ref_stubs  # noqa: E402
from make_golden import npy  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from waymo_eval_ref import iou_pair  # noqa: E402

OUT_DIR = os.path.join(os.environ.get("RV3D_GOLDEN_OUT", HERE), "render")
MAX_SIDE, MPP = 3.0, 0.15
MARGIN = 1e-3
COLS = ("tx_m", "ty_m", "tz_m", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz")


# ---- stand-ins ---------------------------------------------------------------------------------------------------------------
def normalize_min_max(x, min_val: float = 0.0, max_val: float = 1.0, eps: float = 1e-6):
    B, C = x.shape[:2]
    lo = x.reshape(B, C, -1).min(-1).values.view(B, C, 1, 1)
    hi = x.reshape(B, C, -1).max(-1).values.view(B, C, 1, 1)
    return (max_val - min_val) * (x - lo) / (hi - lo + eps) + min_val


def boxes_iou3d(a, b):
    return torch.tensor([[iou_pair(p, q)[1] for q in b.tolist()] for p in a.tolist()], dtype=torch.float32).reshape(len(a), len(b))


def _top_k(self, k, by):
    order = np.argsort(-self._data[by], kind="stable")[:k]
    return self[order]


def install() -> None:
    mod = _ref_stubs._module
    mod("kornia.enhance")
    mod("kornia.enhance.normalize").normalize_min_max = normalize_min_max
    cv2 = mod("cv2")
    cv2.LINE_AA, cv2.FONT_HERSHEY_SIMPLEX = 16, 0
    cv2.polylines = lambda img, *a, **k: img
    cv2.rectangle = lambda img, *a, **k: img
    cv2.putText = lambda img, *a, **k: img
    cv2.getTextSize = lambda *a, **k: ((0, 0), 0)
    mod("torchvision.io")
    mod("torchvision.io.image").write_png = lambda *a, **k: None
    import matplotlib
    import matplotlib.cm

    if not hasattr(matplotlib.cm, "get_cmap"):
        matplotlib.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    sys.modules["mmcv.ops"].boxes_iou3d = boxes_iou3d
    sys.modules["pytorch_lightning"].Trainer = object
    mod("pytorch_lightning.loggers")
    mod("pytorch_lightning.loggers.tensorboard").TensorBoardLogger = type("TensorBoardLogger", (), {})
    mod("pytorch_lightning.loggers.wandb").WandbLogger = type("WandbLogger", (), {})
    mod("pytorch_lightning.trainer")
    mod("pytorch_lightning.trainer.states").RunningStage = types.SimpleNamespace(SANITY_CHECKING="sanity_check")
    mod("pytorch_lightning.utilities")
    mod("pytorch_lightning.utilities.rank_zero").rank_zero_only = lambda fn: fn
    _ref_stubs._PlFrame.top_k = _top_k


install()
from torchbox3d.rendering import tensorboard as ref_tb  # noqa: E402


# ---- margins -----------------------------------------------------------------------------------------------------------------
def bad_index(plane: torch.Tensor, exact: bool = True) -> np.ndarray:
    """Pixels of an fp32 plane whose normalised value times 255 lies within MARGIN of an integer (the exact 0 of the minimum and the
    maximum excepted).  ``exact``: the plane is the same bit for bit in every implementation (norm, abs: IEEE operations only), and so
    is the maximum's index; the maximum of a likelihood plane must sit clear of the next integer by 1e-4 or hit 255 exactly."""
    p = plane.double().numpy()
    lo, hi = p.min(), p.max()
    v = (p - lo) / ((hi - lo) + 1e-6) * 255.0
    d = np.abs(v - np.rint(v))
    top = float(np.float32(np.float32(np.float32(hi - lo) / np.float32(np.float32(hi - lo) + np.float32(1e-6))) * np.float32(255.0)))
    assert exact or hi == lo or top == 255.0 or abs(top - round(top)) > 1e-4, top
    return (d <= MARGIN) & (p != lo) & (p != hi)


def bad_point(cart: torch.Tensor) -> np.ndarray:
    """Pixels of a (3,H,W) fp32 cart whose x or y lands within MARGIN px of a pixel boundary, of the bounds of the view, or on the last
    row / column's far side (where the reference's index store would raise)."""
    c = cart.double().numpy()
    u = (c[:2] + MAX_SIDE) / MPP
    size = MAX_SIDE * 2.0 / MPP
    near = (np.abs(u - np.rint(u)) <= MARGIN) | (np.abs(u) <= MARGIN) | (np.abs(u - size) <= MARGIN)
    return near.any(0) & ((c ** 2).sum(0) > 0)


def settle(sources: dict, bad_of) -> None:
    """``sources``: name -> (C,H,W) tensors that share pixels.  Every bad pixel takes all sources' values of the first good pixel."""
    for _ in range(4):
        bad = bad_of()
        if not bad.any():
            return
        good = np.argwhere(~bad)[0]
        for t in sources.values():
            t[:, torch.from_numpy(bad)] = t[:, good[0], good[1]][:, None]
    assert not bad_of().any()


def grid(t: torch.Tensor, steps: int) -> torch.Tensor:
    return (torch.round(t.double() * steps) / steps).float()


# ---- functions.npz -----------------------------------------------------------------------------------------------------------
def gen_functions() -> dict:
    g = torch.Generator().manual_seed(11)
    out: dict = {"tables/GREYS": ref_tb.GREYS, "tables/TURBO_R": ref_tb.TURBO_R, "tables/VIRIDIS": ref_tb.VIRIDIS,
                 "cfg": np.array([MAX_SIDE, MPP])}
    H, W = 8, 40
    planes = {"random": grid(torch.rand(1, H, W, generator=g, dtype=torch.float64) * 60.0, 256),
              "signed": grid(torch.randn(1, H, W, generator=g, dtype=torch.float64), 1024),
              "constant": torch.full((1, H, W), 2.5),
              "single_max": torch.zeros(1, H, W)}
    planes["single_max"][0, 3, 17] = 7.0
    mask = torch.rand(H, W, generator=g) > 0.3
    for name, p in planes.items():
        settle({"p": p}, lambda p=p: bad_index(p[0]))
        for table in ("GREYS", "TURBO_R", "VIRIDIS"):
            for mname, m in (("masked", mask), ("all_masked", torch.zeros(H, W, dtype=torch.bool)), ("unmasked", None)):
                if mname == "all_masked" and name != "random":
                    continue
                rgb = ref_tb.normalize_apply_colormap(p.clone().view(1, 1, H, W), getattr(ref_tb, table), None if m is None else m.clone())
                assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (3, H, W)
                out[f"colormap/{name}/{table}/{mname}"] = rgb
        out[f"colormap/{name}/plane"] = p[0]
    out["colormap/mask"] = mask
    assert (out["colormap/constant/VIRIDIS/unmasked"].reshape(3, -1) == ref_tb.VIRIDIS[:, :1]).all(), "a constant plane maps to index 0"
    # points: a cloud around the view, the origin (norm 0), points outside on every side
    pts = grid((torch.rand(3, 1, 400, generator=g, dtype=torch.float64) - 0.5) * 7.5, 1024)
    pts[:, 0, :8] = 0.0
    settle({"p": pts}, lambda: bad_point(pts))
    xyz = pts.reshape(3, -1).t().contiguous()
    out["points/xyz"] = xyz
    bev = ref_tb.build_bev(xyz.clone(), MAX_SIDE, MPP)
    side = bev.shape[0]
    assert tuple(bev.shape) == (40, 40, 3) and 50 < int((bev[..., 0] > 0).sum()) < 400
    out["points/bev"] = bev
    w2i = ref_tb.world_to_image(xyz.clone(), MAX_SIDE, MPP)
    assert 0 < len(w2i) < len(xyz) and float(w2i[:, :2].max()) < side
    out["points/world_to_image"] = w2i
    return out


# ---- panels.npz --------------------------------------------------------------------------------------------------------------
def frame(rows: np.ndarray, batch_index, scores=None):
    data = {c: rows[:, i].astype(np.float32) for i, c in enumerate(COLS)}
    if scores is not None:
        data["score"] = np.asarray(scores, np.float32)
    data["batch_index"] = np.asarray(batch_index, np.int32)
    return _ref_stubs._PlFrame(data)


def boxes(g, n: int) -> np.ndarray:
    ctr = (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * 4.0
    z = torch.zeros(n, 1, dtype=torch.float64)
    lwh = torch.tensor([1.0, 0.5, 0.5], dtype=torch.float64) * (1.0 + 0.2 * torch.rand(n, 3, generator=g, dtype=torch.float64))
    yaw = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
    quat = torch.stack([torch.cos(yaw / 2), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.sin(yaw / 2)], 1)
    return grid(torch.cat([ctr, z, lwh, quat], 1), 1024).numpy()


def gen_case(tag: str, seed: int, B: int, H: int, W: int, strides, tasks: dict, aux_keys: dict, out: dict) -> None:
    g = torch.Generator().manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64)
    head, aux = {}, {}
    for s in strides:
        Ws = W // s
        cart = grid((torch.rand(B, 3, H, Ws, **f64) - 0.5) * torch.tensor([9.0, 9.0, 2.0], dtype=torch.float64).view(1, 3, 1, 1), 1024)
        mask = torch.rand(B, 1, H, Ws, generator=g) > 0.2
        cart = cart * mask  # (no return: the point is the origin)
        level = {"cart": cart, "mask": mask}
        shared = {"cart": cart[0]}
        for t, n_cls in tasks.items():
            level[t] = {"logits": grid(torch.randn(B, n_cls, H, Ws, **f64) * 2.0 - 2.0, 64)}
        if s == 1 and aux_keys:
            aux[s] = {t: {k: grid(torch.randn(B, c, H, Ws, **f64), 256) for k, c in aux_keys.items()} for t in tasks}
            aux[s]["mask"] = mask  # (a non-integer key: skipped by the reference)
        # margins of sample 0 (the only one drawn): the planes of this level, and at stride 1 the points
        def bad_of(level=level, s=s, shared=shared):
            bad = bad_index(torch.linalg.norm(level["cart"][0], dim=0))
            if s == 1:
                bad |= bad_point(level["cart"][0])
            for t in tasks:
                bad |= bad_index(level[t]["logits"][0].sigmoid().max(dim=0).values, exact=False)
            if s in aux:
                for t in tasks:
                    for v in aux[s][t].values():
                        for ch in v[0]:
                            bad |= bad_index(ch.abs())
            return bad
        sources = {"cart": level["cart"][0], **{f"l{t}": level[t]["logits"][0] for t in tasks}}
        if s in aux:
            sources.update({f"a{t}{k}": v[0] for t in tasks for k, v in aux[s][t].items()})
        settle(sources, bad_of)
        head[s] = level
    ann_rows, dt_rows = boxes(g, 4), boxes(g, 6)
    annotations = frame(ann_rows, [0, 1, 0, 0])
    dts = frame(dt_rows, [0, 0, 1, 0, 0, 0], scores=[0.5, 0.875, 0.75, 0.25, 0.625, 0.375])
    outputs = {"head": head}
    if aux:
        outputs["aux"] = aux
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self  # (tensorboard.py:300,306: the only device step)
    try:
        images = {"full": ref_tb.draw_detections(dts, None, {"annotations": annotations}, outputs, max_num_dts=3, max_side=MAX_SIDE, meter_per_px=MPP),
                  "no_dts": ref_tb.draw_detections(dts.filter(np.zeros(6, bool)), None, {"annotations": annotations}, outputs, max_side=MAX_SIDE,
                                                   meter_per_px=MPP)}
    finally:
        torch.Tensor.cuda = cuda
    assert torch.equal(images["full"], images["no_dts"]), "with polylines a no-op the detections leave no trace"
    img = images["full"]
    assert img.dtype == torch.uint8 and img.shape[0] == 3
    out[f"{tag}/image"] = img
    out[f"{tag}/strides"] = np.array(list(strides))
    out[f"{tag}/tasks"] = np.array(list(tasks))
    out[f"{tag}/aux_keys"] = np.array(list(aux_keys), dtype="U16")
    for s, level in head.items():
        out[f"{tag}/head/{s}/cart"], out[f"{tag}/head/{s}/mask"] = level["cart"], level["mask"]
        for t in tasks:
            out[f"{tag}/head/{s}/{t}/logits"] = level[t]["logits"]
    for s, entries in aux.items():
        for t in tasks:
            for k, v in entries[t].items():
                out[f"{tag}/aux/{s}/{t}/{k}"] = v
    out[f"{tag}/annotations"] = np.concatenate([ann_rows, np.zeros((4, 2)), np.array([[0], [1], [0], [0]])], 1).astype(np.float32)  # the loader's (M,13)
    out[f"{tag}/dts"], out[f"{tag}/dt_scores"] = dt_rows.astype(np.float32), np.asarray(dts["score"].to_numpy())
    out[f"{tag}/dt_batch_index"] = np.array([0, 0, 1, 0, 0, 0])
    print(tag, tuple(img.shape), "panels", (img.shape[1] - 40) // H)


def gen_panels() -> dict:
    out: dict = {"cfg": np.array([MAX_SIDE, MPP])}
    gen_case("wide", 21, 2, 4, 64, (1, 2), {0: 3, 1: 2}, {"targets": 2, "foreground": 1}, out)
    gen_case("narrow", 22, 2, 4, 37, (1,), {0: 3}, {}, out)
    assert out["wide/image"].shape[2] == 64 and out["narrow/image"].shape[2] == 40
    return out


def main() -> None:
    os.makedirs(OUT_DIR, exist_ok=True)
    for name, arrays in (("functions", gen_functions()), ("panels", gen_panels())):
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, **{k: npy(v) for k, v in arrays.items()})
        size = os.path.getsize(path)
        print(f"render/{name}.npz: {size / 1024:.1f} KiB, {len(arrays)} arrays")
        assert size < 100 * 1024


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
