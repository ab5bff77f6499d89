"""ctypes binding of ``librv3d_hip.so`` (the C ABI declared in ``include/rv3d.h``).

``include/rv3d.h`` is the single source of the binding's types: ``prototypes()`` parses the declarations in its own text once per
process, ``included_prototypes()`` those of the headers it includes (``rv3d_wnms.h``), ``companion_prototypes()`` those of the headers
beside it that include it (``rv3d_render.h``), ``optim_prototypes()`` those of ``rv3d_optim.h`` (another such header: the grouped optimiser
step) and ``average_prototypes()`` the weight-averaging entries of that header, and ``load()`` sets ``restype`` / ``argtypes`` of every
symbol of the five tables.  Call sites pass plain Python values (``int``,
``float``, ``None``, ``ptr(t)``, a ctypes Structure or array); a wrong argument count or a wrong struct raises in Python.

There is deliberately no CPU fallback: if the library is missing or a call fails the host
code raises.  ``load()`` only dlopens the library (works without a GPU, which is what the
CPU test-suite checks); every compute entry point needs a device.
"""

from __future__ import annotations

import ctypes
import os
import re
import functools
from typing import Dict, List, Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RV3D_LIB") or os.path.join(_HERE, "librv3d_hip.so")  # (RV3D_LIB: A/B of two builds in one gpurun call)
# the same sources built with fp16 operands (csrc/common.h, RV_OPERAND_F16): inference under torch.autocast(dtype=float16)
LIB_PATH_F16 = os.environ.get("RV3D_LIB_F16") or os.path.join(_HERE, "librv3d_hip_f16.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "rv3d.h")
# headers beside rv3d.h that include IT and declare further entries of the same library (rv3d_render.h: the debug panels, csrc/render.hip)
COMPANION_HEADERS = ("rv3d_render.h",)
# another header of that kind, with a table of its own (`optim_prototypes()`): the grouped optimiser step of csrc/optim.hip
OPTIM_HEADERS = ("rv3d_optim.h",)
# the weight-averaging entries of that header, a table of their own (`average_prototypes()`): `optim_prototypes()` stays the grouped step
AVERAGE_ENTRIES = ("rv_adamw_step_groups_avg", "rv_average_tensors")

# flags (mirror include/rv3d.h)
IN_AFFINE, IN_RELU, OUT_F32, OUT_BIAS, OUT_STATS, OUT_ACCUM, OUT_RELU = 1, 2, 4, 8, 16, 32, 64
OUT_RES_RELU = 256
WGRAD_TORCH_LAYOUT = 128  # rv_tap_wgrad: result in dT[cu][cv][kh][kw] (no unpack pass)
# kernel-selection hints (rvTapShape.flags, per call: the library keeps no mutable state).  SELECT is OR-ed into every TapShape
# built while a `select(...)` block is active -- the parity tests' way of running the production kernels on crops / pinning a generation.
SEL_SMALL_GRIDS, SEL_SMALL_GRIDS6, SEL_NO_GEN6, SEL_NO_GEN5, SEL_NO_POINTWISE, SEL_NO_POINTWISE_BWD = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25
SELECT = 0
EW_RELU_A, EW_RELU_B, EW_RELU_OUT = 1, 2, 4
BNB_RELU_Z, BNB_RES_ACCUM, BNB_Y_FROM_INPUT = 1, 2, 4
ADAM_AMSGRAD, ADAM_MAXIMIZE = 1, 2  # RV_ADAM_* (rvAdamRow.flags, include/rv3d_optim.h)
WNMS_MERGE_SUPPRESSED, WNMS_SCORE_KEEPER, WNMS_NMS_GE, WNMS_MERGE_GE = 1, 2, 4, 8  # RV_WNMS_* (rv_wnms_opt / rv_nms_sweeps_opt: per call)
# rv_ew_pass_info: passes and kernel forms (RV_EW_PASS_* / RV_EW_FORM_*)
EW_PASS_COMBINE, EW_PASS_MASK_GRAD, EW_PASS_BN_FINALIZE, EW_PASS_BWD_REDUCE, EW_PASS_BWD_REDUCE_PAIR, EW_PASS_BWD_FINALIZE, EW_PASS_BWD_APPLY, EW_PASS_BWD_APPLY_PAIR = range(8)
EW_FORM_COMB, EW_FORM_ROWS, EW_FORM_OCTET, EW_FORM_LEAN, EW_FORM_FUSED_FINALIZE, EW_FORM_TWO_STAGE = range(1, 7)
STATS_SCRATCH_ROWS = 128


class TapGeom(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("kh", "kw", "stride_w", "pad_h", "pad_w", "cu", "cv")]


class TapShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "H", "Wu", "Wv", "ld_src", "ld_dst", "flags")]

    def __init__(self, *args, **kw) -> None:
        super().__init__(*args, **kw)
        self.flags |= SELECT


class select:
    """``with select(SEL_SMALL_GRIDS | ...):`` -- every tap-conv / weight-gradient call issued inside carries these RV_SEL_* hints."""

    def __init__(self, flags: int) -> None:
        self.flags = flags

    def __enter__(self):
        global SELECT
        self.old, SELECT = SELECT, SELECT | self.flags
        return self

    def __exit__(self, *exc):
        global SELECT
        SELECT = self.old


class BnbEpilogue(ctypes.Structure):
    """``rvBnbEpilogue`` of include/rv3d.h (rv_tap_data_grad_bnb)."""

    _fields_ = [("y", ctypes.c_void_p), ("ld_y", ctypes.c_int32), ("flags", ctypes.c_int32), ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p),
                ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p), ("partial", ctypes.c_void_p)]


class TargetLevel(ctypes.Structure):
    """``rvTargetLevel`` of include/rv3d.h (rv_assign_targets_multilevel)."""

    _fields_ = [("stride", ctypes.c_int32), ("use_range", ctypes.c_int32), ("lower", ctypes.c_double), ("upper", ctypes.c_double)]


class TargetOut(ctypes.Structure):
    """``rvTargetOut``: the four target tensors of one (level, task)."""

    _fields_ = [(n, ctypes.c_void_p) for n in ("labels", "panoptics", "reg_targets", "points_per_obj")]


class LossEntry(ctypes.Structure):
    """``rvLossEntry``: the tensors of one (level, task) of the multi-level loss."""

    _fields_ = [(n, ctypes.c_void_p) for n in ("logits", "regressands", "cart", "mask", "labels", "panoptics", "reg_targets", "points_per_obj",
                                               "num_objects", "soft_targets", "foreground", "d_logits", "d_regressands")] + \
               [(n, ctypes.c_int32) for n in ("ld_logits", "ld_reg", "B", "n_cls", "H", "W")]


class LossParams(ctypes.Structure):
    """``rvLossParams``."""

    _fields_ = [("coding_weights", ctypes.c_float * 8)] + [(n, ctypes.c_float) for n in ("cls_weight", "reg_weight", "smoothing", "sigma", "alpha", "gamma")] + \
               [("azimuth_invariant", ctypes.c_int32)]


class LossKinds(ctypes.Structure):
    """``rvLossKinds``: the classification / regression loss of the ``rv_detection_loss_table_*`` pair (``CLS_*`` / ``REG_*``)."""

    _fields_ = [("cls_kind", ctypes.c_int32), ("reg_kind", ctypes.c_int32), ("reg_param", ctypes.c_float)]


class RoiLayer(ctypes.Structure):
    """``rvRoiLayer``: one raster of the ROI atlas (``converters/av2/roi.py``)."""

    _fields_ = [("offset", ctypes.c_int64), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("s", ctypes.c_double), ("tx", ctypes.c_double),
                ("ty", ctypes.c_double)]


class AdamRow(ctypes.Structure):
    """``rvAdamRow`` of include/rv3d_optim.h: the hyper-parameters of one (parameter group, step count) of ``rv_adamw_step_groups``."""

    _fields_ = [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")] + [("step", ctypes.c_int64), ("flags", ctypes.c_int32)]


ML_MAX_LEVELS, ML_MAX_ENTRIES = 8, 16  # RV_ML_MAX_LEVELS / RV_ML_MAX_ENTRIES
AFFINITY_GAUSSIAN, AFFINITY_BEV = 0, 1  # RV_AFFINITY_* (rv_soft_assign)
CLS_VARIFOCAL, CLS_FOCAL, CLS_PENALTY_REDUCED = 0, 1, 2  # RV_CLS_* (rvLossKinds.cls_kind)
REG_L1, REG_SMOOTH_L1, REG_HUBER, REG_MSE = 0, 1, 2, 3  # RV_REG_* (rvLossKinds.reg_kind; reg_param = beta / delta)
EVAL_MAX_THRESHOLDS, EVAL_MAX_DTS = 8, 1024  # RV_EVAL_MAX_* (rv_eval_match)
WAYMO_MAX_DTS, WAYMO_MAX_GTS, WAYMO_MAX_SWEEPS = 1024, 1024, 65536  # RV_WAYMO_MAX_* (rv_waymo_match: per sweep and object type)
WAYMO_NUM_CUTOFFS, WAYMO_NUM_BREAKDOWN_ROWS, WAYMO_NUM_RESULT_ROWS = 101, 16, 32  # RV_WAYMO_NUM_*


def loss_sums_len() -> int:
    """Length of one row of loss sums (``RV_LOSS_SUMS_LEN``), asked of the library."""
    return int(load().rv_detection_loss_sums_len())


class RvError(RuntimeError):
    pass


_lib: Optional[ctypes.CDLL] = None
_lib_f16: Optional[ctypes.CDLL] = None
_OPERAND = "bf16"  # the operand type of the calls being issued: "bf16" (librv3d_hip.so) or "f16" (librv3d_hip_f16.so)


class operand:
    """``with operand("f16"):`` -- every ``call`` / ``load`` inside goes to the fp16-operand build of the library, and
    ``act_dtype()`` is ``torch.float16``.  Set by ``program._ProgramFn`` for an eval-mode program under
    ``torch.autocast(dtype=torch.float16)`` (the reference's ``eval_precision: 16``)."""

    def __init__(self, tag: str) -> None:
        if tag not in ("bf16", "f16"):
            raise RvError(f"unknown operand type {tag!r}")
        self.tag = tag

    def __enter__(self):
        global _OPERAND
        self.old, _OPERAND = _OPERAND, self.tag
        return self

    def __exit__(self, *exc):
        global _OPERAND
        _OPERAND = self.old


def operand_tag() -> str:
    return _OPERAND


def act_dtype() -> "torch.dtype":
    """torch dtype of the 16-bit activation tensors of the current operand type."""
    return torch.float16 if _OPERAND == "f16" else torch.bfloat16


_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = ("void", "float", "double", "uint8_t", "int32_t", "int64_t", "uint64_t")  # T*, const T*, T* const*: all c_void_p
_STRUCTS = {"rvTapGeom": ctypes.POINTER(TapGeom), "rvTapShape": ctypes.POINTER(TapShape), "rvBnbEpilogue": ctypes.POINTER(BnbEpilogue),
            "rvTargetLevel": ctypes.POINTER(TargetLevel), "rvTargetOut": ctypes.POINTER(TargetOut), "rvLossEntry": ctypes.POINTER(LossEntry),
            "rvLossParams": ctypes.POINTER(LossParams), "rvLossKinds": ctypes.POINTER(LossKinds), "rvAdamRow": ctypes.POINTER(AdamRow),
            # fed raw memory: converters/av2/roi.py builds the table as a numpy record array and keeps it in a device tensor
            "rvRoiLayer": ctypes.c_void_p}


def _ctype(decl: str, symbol: str):
    """ctypes type of a parameter / return type as include/rv3d.h spells it."""
    words = decl.replace("*", " * ").split()
    base, depth = [w for w in words if w not in ("const", "*")], words.count("*")
    if len(base) == 1:
        if depth == 0 and base[0] in _SCALARS:
            return _SCALARS[base[0]]
        if (depth == 0 and base[0] == "rvStream") or (depth >= 1 and base[0] in _POINTEES):
            return ctypes.c_void_p
        if depth == 1 and base[0] in _STRUCTS:
            return _STRUCTS[base[0]]
        if words == ["const", "char", "*"]:
            return ctypes.c_char_p
    raise RvError(f"include/rv3d.h: cannot map the type {decl!r} in the declaration of {symbol}")


def _parse_header(path: str) -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\b[^{;]*\{.*?\}[^;]*;", "", text, flags=re.S)
    table = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s*]*?)\b(rv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        plist = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(.*?)\b(\w+)\s*", p, flags=re.S)
            if m is None or not m.group(1).strip():
                raise RvError(f"include/rv3d.h: cannot parse the parameter {p.strip()!r} of {name}")
            plist.append((_ctype(m.group(1), name), m.group(2)))
        table[name] = (_ctype(ret, name), tuple(plist))
    unparsed = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", text)) - set(table)
    if unparsed:
        raise RvError(f"include/{os.path.basename(path)}: cannot parse the declaration of {sorted(unparsed)}")
    return table


@functools.lru_cache(maxsize=None)
def prototypes() -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    """``name -> (restype, ((ctype, parameter name), ...))`` of every function declared in include/rv3d.h itself."""
    return _parse_header(HEADER_PATH)


@functools.lru_cache(maxsize=None)
def included_prototypes() -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    """The same table for the headers that include/rv3d.h pulls in with ``#include "name.h"`` (``rv3d_wnms.h``: the weighted-NMS
    entries with per-call choices), from the directory of the header.  ``load()`` types these entries like the header's own; a
    header that is named but missing is an error."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    table = {}
    for name in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, flags=re.M):
        path = os.path.join(os.path.dirname(HEADER_PATH), name)
        if not os.path.exists(path):
            raise RvError(f"{HEADER_PATH} includes {name!r}, which is missing")
        table.update(_parse_header(path))
    return table


@functools.lru_cache(maxsize=None)
def companion_prototypes() -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    """The same table for ``COMPANION_HEADERS``: headers in include/ that include rv3d.h and declare further entries (``rv3d_render.h``).
    ``load()`` types them like the header's own; one that is missing is an error."""
    return _companion_table(COMPANION_HEADERS)


@functools.lru_cache(maxsize=None)
def optim_prototypes() -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    """The same table for ``OPTIM_HEADERS`` (``rv3d_optim.h``: ``rv_adamw_step_groups``, ``rv_adam_max_rows``)."""
    return {k: v for k, v in _companion_table(OPTIM_HEADERS).items() if k not in AVERAGE_ENTRIES}


@functools.lru_cache(maxsize=None)
def average_prototypes() -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    """The same table for ``AVERAGE_ENTRIES``, declared in ``rv3d_optim.h`` too: the optimiser step that also averages the weights and the
    multi-tensor average (``optim.AveragedModel``).  An entry the header does not declare is an error."""
    table = _companion_table(OPTIM_HEADERS)
    missing = [k for k in AVERAGE_ENTRIES if k not in table]
    if missing:
        raise RvError(f"include/rv3d_optim.h does not declare {missing}")
    return {k: table[k] for k in AVERAGE_ENTRIES}


def _companion_table(names) -> Dict[str, Tuple[object, Tuple[Tuple[object, str], ...]]]:
    table = {}
    for name in names:
        path = os.path.join(os.path.dirname(HEADER_PATH), name)
        if not os.path.exists(path):
            raise RvError(f"the companion header {path} is missing")
        table.update(_parse_header(path))
    return table


def declared_symbols() -> List[str]:
    """Every function name declared in include/rv3d.h (used by the export test)."""
    return sorted(prototypes())


def load(tag: Optional[str] = None) -> ctypes.CDLL:
    global _lib, _lib_f16
    tag = tag or _OPERAND
    if tag == "f16":
        if _lib_f16 is None:
            _lib_f16 = _dlopen(LIB_PATH_F16)
        return _lib_f16
    if _lib is None:
        _lib = _dlopen(LIB_PATH)
    return _lib


def _dlopen(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise RvError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    # Load order matters on a GPU box: the library registers its code objects with the HIP runtime when it is loaded, and
    # it must find the runtime PyTorch already initialised (loaded the other way round -- e.g. build() followed by
    # smoke() in one process -- its launches failed with "no ROCm-capable device is detected").  device_count() does not
    # touch the GPU, so CPU-only boxes (the build check) pass through.
    if torch.cuda.device_count() > 0 and torch.cuda.is_available():
        torch.cuda.init()
    lib = ctypes.CDLL(path)
    # restype / argtypes of every declared symbol; the parameter names make ctypes refuse extra arguments too (a bare cdecl
    # function pointer ignores them) and accept them as keywords
    for name, (restype, params) in {**prototypes(), **included_prototypes(), **companion_prototypes(), **optim_prototypes(), **average_prototypes()}.items():
        try:
            fn = ctypes.CFUNCTYPE(restype, *[t for t, _ in params])((name, lib), tuple((1, p) for _, p in params))
        except AttributeError:
            raise RvError(f"{path} does not export {name}, which include/rv3d.h (or a header it includes, or a companion header) declares") from None
        setattr(lib, name, fn)
    return lib


_DEBUG = bool(int(os.environ.get("RV3D_DEBUG_SYNC", "0")))


# Algorithmic bytes (every operand tensor once in, every result once out, 16-bit activations) of the HBM-bound entry
# points, from their own arguments by the parameter names of include/rv3d.h -- bench.py's `roofline_hbm` prices the group against the
# HBM roofline.
HBM_BYTES = {
    "rv_ew_combine": lambda a: 2.0 * a["pixels"] * a["c"] * (2 + (a["b"] is not None)),
    "rv_bn_bwd_reduce": lambda a: 2.0 * a["pixels"] * a["c"] * (2 + (a["out"] is not None)),
    "rv_bn_bwd_apply": lambda a: 2.0 * a["pixels"] * a["c"] * (3 + (a["out"] is not None) + 2 * (a["dres"] is not None)),
    "rv_bn_bwd_reduce_pair": lambda a: 2.0 * a["pixels"] * a["c"] * 4,
    "rv_bn_bwd_apply_pair": lambda a: 2.0 * a["pixels"] * a["c"] * 6,
    # MetaKernel stem: pixels = N H W, the 9x-grid tensors hold 9 C values per pixel
    "rv_meta_modulate": lambda a: 2.0 * a["N"] * a["H"] * a["W"] * a["C"] * 19,
    "rv_meta_modulate_bwd_sums": lambda a: 2.0 * a["N"] * a["H"] * a["W"] * a["C"] * 20,
    "rv_meta_modulate_bwd_apply": lambda a: 2.0 * a["N"] * a["H"] * a["W"] * a["C"] * 28,
    "rv_pos_forward": lambda a: float(a["pixels"]) * (16 + 4.0 * a["c"]),
    "rv_pos_backward_sums": lambda a: float(a["pixels"]) * (16 + 2.0 * a["c"]),
    # final conv of a tower fused with the BatchNorm backward in front of it: y (+ the 32-channel dY) in; _apply also writes dy
    "rv_head_final_bwd_sums": lambda a: 2.0 * a["pixels"] * (a["c"] + 32),
    "rv_head_final_bwd_apply": lambda a: 2.0 * a["pixels"] * (2 * a["c"] + 32),
}
HBM_HOOK = None  # callable(name, algorithmic bytes, launch) or None: set by bench.py around its HBM-group measurement


def call(name: str, *args) -> None:
    """Invoke an int-returning entry point; raise with rv_last_error() on failure.

    ``RV3D_DEBUG_SYNC=1`` prints every call and synchronises after it (locates a faulting launch).
    """
    if HBM_HOOK is not None and name in HBM_BYTES:
        hook, nbytes = HBM_HOOK, HBM_BYTES[name](dict(zip((p for _, p in prototypes()[name][1]), args)))
        return hook(name, nbytes, lambda: _call(name, *args))
    return _call(name, *args)


def _call(name: str, *args) -> None:
    fn = getattr(load(), name)
    if _DEBUG:
        import sys

        import torch

        print(f"[rv3d] {name}", file=sys.stderr, flush=True)
    rc = fn(*args)
    if rc != 0:
        raise RvError(f"{name} failed: {load().rv_last_error().decode()}")
    if _DEBUG:
        torch.cuda.synchronize()


def tap_launch_info(geom: TapGeom, shape: TapShape, scatter: bool):
    """``rv_tap_launch_info``: (kernel generation, variant, grid.x, grid.y) of the launch the library plans for this tap op, or ``None``
    when it rejects the shape (``rv_last_error`` says why).  Launches nothing."""
    info = (ctypes.c_int32 * 4)()
    if load().rv_tap_launch_info(geom, shape, 1 if scatter else 0, info) != 0:
        return None
    return tuple(info)


def ew_pass_info(pass_id: int, pixels_or_rows: int, c: int, ld=None, has_out: bool = False, has_dres: bool = False, flags: int = 0):
    """``rv_ew_pass_info``: (form, non-temporal, grid, template index) of the launch the library plans for a BatchNorm / element-wise
    pass at this shape -- the plan the entry point itself launches from.  ``ld``: the row pitches in the entry point's argument order
    (reduce: dout, out, y; reduce_pair: dout, out, ya, yb; apply: dout, out, y, dy, dres), ``None`` = all ``c``.  Launches nothing;
    raises ``RvError`` on a shape the library rejects."""
    info = (ctypes.c_int32 * 4)()
    lds = (ctypes.c_int32 * 5)(*(list(ld) + [0] * (5 - len(ld)))) if ld is not None else None
    if load().rv_ew_pass_info(pass_id, pixels_or_rows, c, lds, 1 if has_out else 0, 1 if has_dres else 0, flags, info) != 0:
        raise RvError(f"rv_ew_pass_info failed: {load().rv_last_error().decode()}")
    return tuple(info)


def ptr(t) -> Optional[ctypes.c_void_p]:
    """Device (or host) pointer of a torch tensor; ``None`` (NULL) for ``None``, which is what ``HBM_BYTES`` tests."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr() -> ctypes.c_void_p:
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# the scalar types by their short names, for callers that build a ctypes array or an out-parameter (`f32 * 5`, a by-reference count);
# no argument needs them: load() types every parameter
i32 = ctypes.c_int32
i64 = ctypes.c_int64
f32 = ctypes.c_float
f64 = ctypes.c_double
