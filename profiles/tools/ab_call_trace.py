"""Every C-ABI call of one training step, as text, to diff between two checkouts that load the SAME built libraries (RV3D_LIB /
RV3D_LIB_F16): ``_lib._call`` is wrapped to log the entry-point name, every non-pointer argument (structures field by field;
pointers only as ptr / null) and whether the current stream is the weight-gradient side stream.  One step (forward, loss, backward)
of the tiny golden detector and of the rv-av2 / rv-waymo / base-av2 widths on the crops of tests/test_gpu_realwidth.py with 2 sweeps,
once in the default mode and once on the one-rank SyncBN path of tests/test_gpu_ddp.py; one file per case, OUT_DIR/<mode>_<case>.txt.
In the default mode also the ``lifecycle`` case (the c32 detector at 2 x 16 x 64 and rv-av2 on its crop): training step (with the fused
optimiser step), training step, eval forward in bf16, eval forward under autocast(float16), training step, eval forward in bf16, in one
process -- every weight-image pack launch (``rv_pack_weight*``, ``rv_pack_batch*``) is in it, with the steps marked.  ``prepack_stale``
orders the table of ``rv_pack_batch`` by ``id()`` of the layers, an address: each run of ``rv_pack_batch_fill`` / ``_fill_folded`` lines is
written sorted, so that two processes can be compared.

    python profiles/tools/ab_call_trace.py OUT_DIR [TREE]      TREE: the checkout to trace (default: the one this file is in)
    diff -r OUT_DIR_A OUT_DIR_B

Each mode runs in a child process of its own (the SyncBN switches are read when the engine is imported).
"""

import contextlib
import ctypes
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = (("rv-av2", 5, 26, 256), ("rv-waymo", 6, 3, 336), ("base-av2", 5, 26, 256))  # (widths, features, classes, W)


def _fmt(a, ctype=None):
    if isinstance(a, ctypes.Structure):
        return "{" + " ".join(f"{n}={_fmt(getattr(a, n), t)}" for n, t in a._fields_) + "}"
    if ctype is not None and (ctype is ctypes.c_void_p or issubclass(ctype, ctypes._Pointer)):
        return "ptr" if a else "null"
    if isinstance(a, ctypes.Array) and ctype is not None:  # (an array FIELD is data; an array argument is an out-parameter)
        return "[" + " ".join(repr(x) for x in a) + "]"
    if a is None or (isinstance(a, ctypes.c_void_p) and not a.value):
        return "null"
    if isinstance(a, (bool, int, float, str, bytes)):
        return repr(a)
    if isinstance(a, ctypes._SimpleCData) and not isinstance(a, ctypes.c_void_p):
        return repr(a.value)
    return "ptr"  # c_void_p, byref(...), ctypes arrays and pointers


def sorted_fill_runs(lines):
    """``lines`` with every run of consecutive calls of one ``rv_pack_batch_fill*`` entry point sorted (their order is an address order)."""
    out, i = [], 0
    while i < len(lines):
        name, j = lines[i].split(" ", 1)[0], i + 1
        while name.startswith("rv_pack_batch_fill") and j < len(lines) and lines[j].split(" ", 1)[0] == name:
            j += 1
        out += sorted(lines[i:j])
        i = j
    return out


def child(out_dir: str, tree: str, mode: str) -> None:
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    if mode == "syncbn":
        os.environ.update(RV3D_SYNC_WORLD1="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29677", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import numpy as np
    import torch

    import bench
    import test_gpu_model as TM
    import test_gpu_realwidth as RW
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd import engine as E

    dev = torch.device("cuda:0")
    if mode == "syncbn":
        torch.distributed.init_process_group("nccl", device_id=dev, rank=0, world_size=1)
        E.SYNC_BN = True
    lines, real = [], L._call

    def traced(name, *args):
        cur = torch.cuda.current_stream().cuda_stream
        side = any(s.cuda_stream == cur for s in E._SIDE_STREAMS.values())
        lines.append(f"{name} {'side' if side else 'main'} " + " ".join(_fmt(a) for a in args))
        return real(name, *args)

    def step(case, backbone, head, data):
        del lines[:]
        L._call = traced
        try:
            feats = backbone(data)
            _, losses = head(feats, data, return_loss=True)
            lines.append("-- backward --")
            losses["loss"].backward()
            torch.cuda.synchronize()
        finally:
            L._call = real
        with open(os.path.join(out_dir, f"{mode}_{case}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{mode} {case}: {len(lines) - 1} calls, loss {float(losses['loss'].detach()):.6f}", flush=True)

    def lifecycle(case, model, data):
        from range_view_3d_detection_amd.optim import AdamW

        def train():
            model.train()
            opt.zero_grad(set_to_none=True)
            model(data).backward()
            opt.step()

        def evaluate(cast):
            model.eval()
            with torch.no_grad(), cast:
                model.head(model.backbone(data), data, return_loss=False)

        opt = AdamW(list(model.parameters()), lr=1e-3)
        bf16, f16 = contextlib.nullcontext(), torch.autocast("cuda", dtype=torch.float16)
        del lines[:]
        L._call = traced
        try:
            for what, run in (("train", train), ("train", train), ("eval bf16", lambda: evaluate(bf16)), ("eval f16", lambda: evaluate(f16)),
                              ("train", train), ("eval bf16", lambda: evaluate(bf16))):
                lines.append(f"-- {what} --")
                run()
            torch.cuda.synchronize()
        finally:
            L._call = real
        with open(os.path.join(out_dir, f"{mode}_lifecycle_{case}.txt"), "w") as f:
            f.write("\n".join(sorted_fill_runs(lines)) + "\n")
        print(f"{mode} lifecycle {case}: {len(lines) - 6} calls", flush=True)

    z = np.load(os.path.join(tree, "tests", "golden", "tiny_model.npz"))
    g = {k: torch.from_numpy(np.asarray(z[k])) for k in z.keys()}
    backbone, head = TM.build_tiny()
    backbone.load_state_dict({k[len("sd/backbone."):]: v for k, v in g.items() if k.startswith("sd/backbone.")})
    head.load_state_dict({k[len("sd/head."):]: v for k, v in g.items() if k.startswith("sd/head.")})
    data = {"features": g["features"].to(dev), "cart": g["cart"].to(dev), "mask": g["mask"].to(dev), "annotations": g["annotations"]}
    step("tiny", backbone.to(dev).train(), head.to(dev).train(), data)
    for widths, n_feat, n_cls, W in CASES:
        backbone, head, _, batch = RW._prepare(widths, n_feat, n_cls, W, 3.0, B=2)
        model = bench.Detector(backbone, head).to(dev).train()
        data = {k: (v.to(dev) if k != "annotations" else v) for k, v in batch.items()}
        with RW._small_grids(True):  # (crops: the production kernels, as in the test)
            step(widths, model.backbone, model.head, data)
            if mode == "default" and widths == "rv-av2":
                lifecycle(widths, model, data)
    if mode == "default":
        torch.manual_seed(0)
        model = bench.Detector(*bench.build_model("c32", 3)).to(dev)
        lifecycle("c32", model, bench.synthetic_batch(2, 16, 64, seed=3, device=dev, boxes_per_sweep=4, n_cls=3))
    if mode == "syncbn":
        torch.distributed.destroy_process_group()


def main() -> None:
    if len(sys.argv) > 3:
        return child(*sys.argv[1:4])
    out_dir = os.path.abspath(sys.argv[1])
    tree = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else HERE
    os.makedirs(out_dir, exist_ok=True)
    for mode in ("default", "syncbn"):
        subprocess.run([sys.executable, os.path.abspath(__file__), out_dir, tree, mode], check=True)


if __name__ == "__main__":
    main()
