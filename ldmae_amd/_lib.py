"""ctypes binding of libldmae_hip.so (include/ldmae_hip.h).

There is NO fallback: if the shared library is missing or a call fails the
caller gets a RuntimeError.  torch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libldmae_hip.so")
LIB_PATH = os.environ.get("LDMAE_HIP_LIB", LIB_PATH)      # A/B builds of the same library (tools/); unset = the in-tree build

F32, BF16, F16 = 0, 1, 2
EPI_BIAS, EPI_GATE_RES, EPI_BIAS_POS, EPI_BIAS_GELU, EPI_SWIGLU, EPI_SWIGLU_BWD, EPI_GELU_BWD = 0, 1, 2, 3, 4, 5, 6

_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float,
            "double": C.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "const char*": C.c_char_p})


def parse_header(text: str) -> dict:
    """name -> (restype, [argtypes]) of every prototype in a C header that holds nothing but plain C89 prototypes, comments, preprocessor
    lines and the extern "C" braces.  Scalars map to their ctypes type, every pointer parameter to c_void_p (device pointers are integers;
    host arrays and byref() pass as well), a `const char*` return to c_char_p, a `void` return to None.  STRICT: a type outside that
    list, or text that is no prototype, raises ValueError with the offending declaration -- nothing ever defaults to int."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", text)
    sigs = {}
    for decl in text.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"([\w ]+?\*?) ?(\w+) ?\(([^()]*)\)", decl)
        if m is None:
            raise ValueError(f"not a C prototype: {decl!r}")
        ret, name, params = m.group(1).strip().replace(" *", "*"), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise ValueError(f"return type {ret!r} has no ctypes mapping: {decl!r}")
        args = []
        for prm in ([] if params == "void" else params.split(",")):
            ctype = " ".join(w for w in prm.split()[:-1] if w != "const")          # the last word is the parameter's name
            if "*" not in prm and ctype not in _SCALARS:
                raise ValueError(f"parameter {prm.strip()!r} has no ctypes mapping: {decl!r}")
            args.append(C.c_void_p if "*" in prm else _SCALARS[ctype])
        sigs[name] = (_RETURNS[ret], args)
    return sigs


def _parse_file(*parts):
    with open(os.path.join(_HERE, *parts)) as f:
        return parse_header(f.read())


# name -> (restype, [argtypes]), derived from the headers at import: the headers are the only place a signature is written down
SIGNATURES = _parse_file("..", "include", "ldmae_hip.h")
# csrc/probe/ldmae_diag.h: present only in the diagnostic build (LDMAE_HIP_LIB=.../libldmae_hip_diag.so, used by tools/)
DIAG_SIGNATURES = _parse_file("csrc", "probe", "ldmae_diag.h")
EPI_TILE_LAUNCH = 0x100
EPI_HALF_LINES = 0x200
EPI_F16_INF = 0x400

_lib = None


def load():
    """dlopen the library (once) and declare every prototype.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ldmae_amd/csrc`).  ldmae_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if hasattr(lib, "ldmae_tune"):          # diagnostic build: LDMAE_TUNE="key=value,..." presets its A/B knobs for profiling runs
        for name, (res, args) in DIAG_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for kv in filter(None, os.environ.get("LDMAE_TUNE", "").split(",")):
            k, v = kv.split("=")
            if lib.ldmae_tune(int(k), int(v)) != 0:
                raise RuntimeError(f"LDMAE_TUNE={kv!r}: {lib.ldmae_last_error().decode()}")
    elif os.environ.get("LDMAE_TUNE"):
        raise RuntimeError("LDMAE_TUNE is set but the loaded library has no A/B knobs: point LDMAE_HIP_LIB at "
                           "ldmae_amd/libldmae_hip_diag.so (make -C ldmae_amd/csrc diag)")
    _lib = lib
    return lib


def last_error() -> str:
    return load().ldmae_last_error().decode()


def call(name, *args):
    """Invoke an int-returning entry point; raise RuntimeError with the library's message on failure."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {last_error()}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL); raises for a tensor off the HIP device.  The LAYOUT is not checked here: the address
    is that of the first element, and the strides the kernel assumes are the caller's to guarantee (ops.py checks them per argument)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("ldmae_amd ops need tensors on a HIP device (no CPU fallback); got " + str(t.device))
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt(dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float16:          # the TF32-class forward path (LDMAE_F16: forward-only entry points)
        return F16
    raise RuntimeError(f"unsupported activation dtype {dtype} (float32, bfloat16, or float16 on the forward-only TF32-class path)")


COUNT_NAMES = ("nt_bf16", "nt_f32", "tn_bf16", "tn_f32", "attn_bf16", "attn_f32", "nt_f16", "attn_f16", "tn_f16")


def launch_counts(reset: bool = False) -> dict:
    """Launch counts by kernel family since the last reset (ldmae_launch_counts): which arithmetic type the calls were dispatched to."""
    arr = (C.c_long * 9)()
    call("ldmae_launch_counts", arr, 9, 1 if reset else 0)
    return dict(zip(COUNT_NAMES, [int(v) for v in arr]))


MX8_COUNT_NAMES = ("quantize", "norm_quantize", "gemm")


def mx8_launch_counts(reset: bool = False) -> dict:
    """Launch counts of the MXFP8 sampling mode since the last reset (ldmae_mx8_launch_counts; separate from launch_counts)."""
    arr = (C.c_long * 3)()
    call("ldmae_mx8_launch_counts", arr, 3, 1 if reset else 0)
    return dict(zip(MX8_COUNT_NAMES, [int(v) for v in arr]))
