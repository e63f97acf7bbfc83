"""ctypes bindings to ``_lib/libpda_kernels.so`` (the gfx950 HIP kernels).

The library exposes a C ABI of launchers that take raw device pointers and a
``hipStream_t``; no torch headers are compiled, so the build is fast and
ABI-independent of the PyTorch wheel. That ABI is declared once, in
``csrc/pda_api.h``: the compiler holds every definition to it, and :func:`load`
binds ``argtypes`` / ``restype`` from the same text (:func:`read_api`). Every
launcher returns the HIP error code of the launch, which :func:`check` turns into
an exception -- ops never fall back silently to PyTorch on a GPU box (a missing
library raises).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path
from types import SimpleNamespace
from typing import Optional

import torch

__all__ = ["load", "available", "lib", "has", "DT", "dt_of", "ConvDesc", "BwdArgs", "BnEpi", "BnFwdOut",
           "BnBwdOut", "RedDescC", "SegRow", "BlkRow", "EmaRange", "stream", "ptr"]

_LIB: Optional[SimpleNamespace] = None
_ERR: Optional[str] = None
API_H = Path(__file__).resolve().parent.parent / "csrc" / "pda_api.h"
LIBPATH = Path(__file__).resolve().parent.parent / "_lib" / "libpda_kernels.so"
if os.environ.get("PDA_KERNEL_LIB"):   # A/B variants (tools/build_variant.py), relative to _lib/
    LIBPATH = LIBPATH.parent / os.environ["PDA_KERNEL_LIB"]

DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def dt_of(t) -> int:
    return DT[t if isinstance(t, torch.dtype) else t.dtype]


# ------------------------------------------------------------------ the structs of csrc/pda_api.h
# (field for field; tests/test_abi_cpu.py holds each layout to the header's static_asserts)
class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("Nb", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "Ho", "Wo")]


class BwdArgs(C.Structure):
    """``BwdArgsC``: arguments of pda_bn_bwd_reduce / pda_bn_bwd_apply."""
    _fields_ = [("g1", C.c_void_p), ("g2", C.c_void_p), ("gp", C.c_void_p), ("HW", C.c_int),
                ("y", C.c_void_p), ("sc", C.c_void_p), ("sh", C.c_void_p),
                ("y2", C.c_void_p), ("sc2", C.c_void_p), ("sh2", C.c_void_p),
                ("mode", C.c_int), ("dz_out", C.c_void_p),
                ("part", C.c_void_p), ("nq", C.c_int), ("rows", C.c_longlong), ("C", C.c_int)]


class BnEpi(C.Structure):
    """dgrad epilogue = BatchNorm-backward reduction (csrc/conv_gemm.hip ConvParams e*)."""
    _fields_ = [("mode", C.c_int), ("nq", C.c_int),
                ("y", C.c_void_p), ("sc", C.c_void_p), ("sh", C.c_void_p),
                ("y2", C.c_void_p), ("sc2", C.c_void_p), ("sh2", C.c_void_p),
                ("g2", C.c_void_p), ("part", C.c_void_p), ("mask", C.c_void_p)]


class BnFwdOut(C.Structure):
    """Outputs of the one-launch BatchNorm forward statistics (csrc/bn.hip bn_stats_kernel<0>)."""
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("eps", C.c_float), ("momentum", C.c_float),
                ("mean", C.c_void_p), ("invstd", C.c_void_p), ("scale", C.c_void_p),
                ("shift", C.c_void_p), ("rmean", C.c_void_p), ("rvar", C.c_void_p),
                ("nbt", C.c_void_p), ("update", C.c_int), ("tot", C.c_void_p)]


class BnBwdOut(C.Structure):
    """Outputs of the one-launch BatchNorm backward finalize (csrc/bn.hip bn_stats_kernel<1>):
    branch 0 = the BN of y, branch 1 = the shortcut BN of y2; k = [branches][3][C]."""
    _fields_ = [("count", C.c_float), ("gscale", C.c_float), ("accumulate", C.c_int),
                ("gamma", C.c_void_p * 2), ("mean", C.c_void_p * 2), ("invstd", C.c_void_p * 2),
                ("dgamma", C.c_void_p * 2), ("dbeta", C.c_void_p * 2), ("k", C.c_void_p)]


class RedDescC(C.Structure):
    """One split-K reduction of pda_wgrad_reduce_batch."""
    _fields_ = [("slab", C.c_void_p), ("grad", C.c_void_p), ("ck", C.c_void_p), ("cB", C.c_void_p),
                ("cs", C.c_void_p)] + [(n, C.c_int) for n in
                                       ("splits", "M", "N", "cin_log2", "cin_real", "pitch",
                                        "accumulate")] + [("scale", C.c_float)]


class SegRow(C.Structure):
    """One parameter tensor's range of the flat buffers and its hyper-parameters (csrc/optim.hip)."""
    _fields_ = [("off", C.c_longlong), ("numel", C.c_longlong), ("lr", C.c_float),
                ("momentum", C.c_float), ("wd", C.c_float), ("trust", C.c_float), ("eps", C.c_float),
                ("flags", C.c_int), ("blk0", C.c_int), ("nblk", C.c_int)]


class BlkRow(C.Structure):
    """One block's chunk: ``count`` <= SEG_CHUNK elements of segment ``seg`` from flat index ``first``."""
    _fields_ = [("first", C.c_longlong), ("seg", C.c_int), ("count", C.c_int)]


class EmaRange(C.Structure):
    """One (e, p[, 16-bit shadow of p]) range of ``count`` 4-byte elements (csrc/ema.hip)."""
    _fields_ = [("e", C.c_void_p), ("p", C.c_void_p), ("shadow", C.c_void_p), ("count", C.c_longlong)]


STRUCTS = {"ConvDesc": ConvDesc, "BwdArgsC": BwdArgs, "BnEpi": BnEpi, "BnFwdOut": BnFwdOut,
           "BnBwdOut": BnBwdOut, "RedDescC": RedDescC, "SegRow": SegRow, "BlkRow": BlkRow,
           "EmaRange": EmaRange}
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double,
            "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}
_HANDLES = ("hipStream_t", "hipEvent_t")


# ------------------------------------------------------------------ reading csrc/pda_api.h
def _ctype(decl: str):
    """The ctypes type of one named parameter (``const float* x``) in the header's restricted style."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    base, stars = " ".join(w for w in words[:-1] if w != "*"), words[:-1].count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base in _HANDLES:
        return C.c_void_p
    if stars == 1 and base in STRUCTS:
        return C.POINTER(STRUCTS[base])
    if stars == 1 and (base in _SCALARS or base in _HANDLES or base == "void"):
        return C.c_void_p
    raise ValueError(f"pda_api.h: parameter {decl!r} is outside the types the header may use")


def _code(text: str) -> str:
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def read_api(text: str) -> dict:
    """``{name: (restype, [argtypes])}`` of every ``pda_*`` prototype in the header text."""
    api = {}
    for ret, name, params in re.findall(r"^[ \t]*(\w[\w ]*?) +(pda_\w+)\(([^)]*)\);", _code(text), re.M):
        if ret not in _SCALARS:
            raise ValueError(f"pda_api.h: {name} returns {ret!r}")
        api[name] = (_SCALARS[ret], [_ctype(p) for p in params.split(",") if p.strip()])
    return api


def read_layouts(text: str) -> dict:
    """``{struct: (sizeof, last field, its offset)}`` from the header's static_asserts."""
    code = _code(text)
    size = dict(re.findall(r"static_assert\(sizeof\((\w+)\) == (\d+)", code))
    return {s: (int(size[s]), f, int(o))
            for s, f, o in re.findall(r"static_assert\(offsetof\((\w+), (\w+)\) == (\d+)", code)}


def api_text() -> str:
    return API_H.read_text()


def stream_cfg() -> tuple:
    """16-bit BN apply passes (csrc/bn.hip StreamCfg): 4 chunks per thread + nontemporal loads /
    stores for tensors >= 50 MiB, the one-chunk kernels below, grid cap 65536 blocks. In-step A/B
    (tools/gpu_ab.sh, one box): 30.02 ms (one-chunk everywhere) vs 29.41 ms (100 MiB threshold);
    threshold 200 / 100 / 50 / 30 MiB: 29.38-29.53 / 29.16 / 29.06-29.11 / 29.02-29.13 ms; grid cap
    8192 / 16384 / 32768 / 65536: 29.53 / 29.15-29.27 / 28.90-29.09 / 28.86-28.97 ms."""
    # memory policy bits: 1 nontemporal loads, 2 nontemporal stores (write-through sc1 stores, bit
    # 4, measured +0.27 ms/step: profiles/ab_r4.md section 1)
    return (-1, 3, 65536, 50)


def load(required: bool = False) -> Optional[SimpleNamespace]:
    """The bound library: a namespace holding exactly the functions pda_api.h declares, so a name it
    does not declare fails in Python (AttributeError) instead of reaching C without ``argtypes``."""
    global _LIB, _ERR
    if _LIB is not None:
        return _LIB
    if not LIBPATH.exists() and os.environ.get("PDA_NO_BUILD") != "1":
        try:
            from .. import _build
            _build.build_kernels()
        except Exception as e:  # pragma: no cover
            _ERR = f"build failed: {e}"
    try:
        dll = C.CDLL(str(LIBPATH))
    except OSError as e:
        _ERR = str(e)
        if required:
            raise RuntimeError(f"native kernels unavailable: {_ERR}") from e
        return None
    lib = SimpleNamespace()
    for name, (restype, argtypes) in read_api(api_text()).items():
        fn = getattr(dll, name, None)
        if fn is None:
            if os.environ.get("PDA_KERNEL_LIB"):   # an A/B variant library may hold a subset
                continue
            raise RuntimeError(f"{LIBPATH} lacks {name}, which csrc/pda_api.h declares: rebuild it")
        fn.argtypes, fn.restype = argtypes, restype
        setattr(lib, name, fn)
    if hasattr(lib, "pda_set_stream_cfg"):
        lib.pda_set_stream_cfg(*stream_cfg())
    _LIB = lib
    return _LIB


def available() -> bool:
    return load() is not None


def lib() -> SimpleNamespace:
    l = load(required=True)
    assert l is not None
    return l


def has(name: str) -> bool:
    """Whether the loaded library has ``name`` (an A/B variant library may lack some launchers)."""
    return hasattr(lib(), name)


def stream(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with HIP error {rc}")
