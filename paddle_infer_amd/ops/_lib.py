"""ctypes binding of the in-tree HIP kernel library ``_lib/libpiamd_kernels.so``.

The entry points and their signatures are read from the library's own header,
``csrc/kernels/piamd_kernels.h``; only the argument-block structs are mirrored here by hand.

The library is loaded lazily, *after* ``import torch`` so that its ``libamdhip64.so.7`` dependency
resolves to the HIP runtime torch already mapped (one runtime, one set of streams). Every launch
goes onto torch's current HIP stream, so the kernels compose with hipBLASLt GEMMs, RCCL
collectives on side streams and ``torch.cuda.CUDAGraph`` (hipGraph) capture.

Dispatch rule used by every op module: a tensor on the GPU runs the HIP kernel and FAILS LOUDLY
if the library is missing; CPU tensors take the PyTorch reference path (used by the CPU test tier
and as the numerics reference of the GPU tests).
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

import torch

from .. import _build

_LIB = None
_LOCK = threading.Lock()
# the one declaration of the library's C ABI; argtypes / restype are read from it at load time
HEADER = os.path.join(_build.KDIR, "piamd_kernels.h")

c_void_p, c_int, c_float, c_ll, c_u64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                         ctypes.c_longlong, ctypes.c_uint64)


class FaArgs(ctypes.Structure):
    """Mirror of ``struct FaArgs`` (csrc/kernels/fa_args.h)."""
    _fields_ = ([(n, c_void_p) for n in ("q", "k", "v", "o", "lse", "dout", "delta", "dq", "dk", "dv",
                                        "mask", "cu_q", "cu_k")]
                + [(n, c_int) for n in ("B", "Sq", "Sk", "Hq", "Hk", "D", "ltot", "causal")]
                + [(n, c_ll) for n in ("sqb", "sqs", "sqh", "skb", "sks", "skh", "svb", "svs", "svh",
                                       "sob", "sos", "soh", "smb", "smh", "smq")]
                + [("scale", ctypes.c_float), ("p_drop", ctypes.c_float), ("seed", c_u64),
                   ("offset", c_u64), ("map", c_int), ("ds", c_void_p)])


class MegaArgs(ctypes.Structure):
    """Mirror of ``struct MegaArgs`` (csrc/kernels/decode_args.h)."""
    _fields_ = ([("layers", c_void_p)] + [(n, c_int) for n in ("nl", "maxS", "nsplit", "act")]
                + [("eps", ctypes.c_float), ("scale_log2", ctypes.c_float)]
                + [(n, c_void_p) for n in ("resid", "rbuf", "qn", "kvn", "part", "h", "bar", "err",
                                        "pos", "trace")] + [("late_dma", c_int), ("loader", c_int)]
                + [("rot", c_int), ("neox", c_int), ("log2_base", ctypes.c_float), ("w8", c_int),
                   ("nb", c_int), ("mm", c_int)])


class HeadArgs(ctypes.Structure):
    """Mirror of ``struct HeadArgs`` (csrc/kernels/decode_args.h)."""
    _fields_ = ([(n, c_void_p) for n in ("y", "g", "b")] + [("eps", ctypes.c_float), ("V", c_int)]
                + [(n, c_void_p) for n in ("w", "best", "cnt", "out", "done")]
                + [("eos", ctypes.c_longlong), ("pad", ctypes.c_longlong)]
                + [(n, c_void_p) for n in ("pos", "tok", "wemb", "pemb")]
                + [("P", c_int), ("resid", c_void_p)])


_SCALARS = {"int": c_int, "float": c_float, "long long": c_ll, "uint64_t": c_u64,
            "unsigned long long": c_u64, "hipStream_t": c_void_p}
_STRUCTS = {"FaArgs": FaArgs, "MegaArgs": MegaArgs, "HeadArgs": HeadArgs}
_DECL = re.compile(r"PIAMD_EXPORT\s+([\w\s]+?)\s*\b(piamd_\w+)\s*\(([^)]*)\)\s*;")


def _ctype(decl: str, entry: str):
    """ctypes type of a C type as ``entry``'s declaration spells it (``const`` dropped)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    base = " ".join(words[:words.index("*")] if "*" in words else words)
    if "*" in words:
        if base == "char":
            return ctypes.c_char_p
        return ctypes.POINTER(_STRUCTS[base]) if base in _STRUCTS else c_void_p
    if base not in _SCALARS:
        raise TypeError(f"{entry}: no ctypes mapping for the C type {decl.strip()!r}")
    return _SCALARS[base]


def parse_header(path: str) -> dict:
    """``{name: (restype, argtypes)}`` of every ``PIAMD_EXPORT <ret> piamd_<name>(<params>);``."""
    with open(path, encoding="utf-8") as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    sigs = {}
    for ret, name, params in _DECL.findall(text):
        params = [p for p in params.split(",") if p.strip() and p.strip() != "void"]
        # a parameter is `<type> <name>`: the type is everything before the last identifier
        sigs[name] = (_ctype(ret, name), [_ctype(re.sub(r"\w+\s*$", "", p), name) for p in params])
    return sigs


class _Kernels:
    """The entry points the header declares, each bound to its symbol with argtypes and restype
    set, as attributes; any other name raises (no call ever goes through ctypes' defaults)."""

    def __init__(self, path: str, header: str):
        self._cdll = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        for name, (restype, argtypes) in parse_header(header).items():
            try:
                fn = getattr(self._cdll, name)
            except AttributeError:
                raise ImportError(f"{path} has no symbol {name}, which {header} declares: the library "
                                  "is stale, rebuild it with `python -m paddle_infer_amd._build`") from None
            fn.restype, fn.argtypes = restype, argtypes
            setattr(self, name, fn)

    def __getattr__(self, name):  # reached only for names that were not bound above
        raise AttributeError(f"{name} is not an entry point declared in {os.path.basename(HEADER)}")


def lib_path() -> str:
    # PIAMD_KERNEL_LIB: load another build of the kernel library (A/B timing of a kernel edit)
    return os.environ.get("PIAMD_KERNEL_LIB") or _build.KERNEL_LIB


def _load(header: str = HEADER) -> _Kernels:
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"paddle_infer_amd HIP kernel library not built ({path}); run "
            "`python -m paddle_infer_amd._build` (or __graft_entry__.build()).")
    return _Kernels(path, header)


def lib() -> _Kernels:
    global _LIB
    if _LIB is None:
        with _LOCK:
            if _LIB is None:
                _LIB = _load()
    return _LIB


def available() -> bool:
    try:
        lib()
        return True
    except (RuntimeError, OSError):
        return False


def has(name: str) -> bool:
    return hasattr(lib(), name)


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def call(name: str, *args) -> None:
    fn = getattr(lib(), name)
    err = fn(*args)
    if err != 0:
        raise RuntimeError(f"{name} failed with hipError {err}")


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def dtype_code(t: torch.Tensor, fp16: bool = False) -> int:
    """Kernel dtype code: 0 = f32, 1 = bf16, 2 = fp16 (only for kernels built for it: ``fp16=True``)."""
    if t.dtype == torch.bfloat16:
        return 1
    if t.dtype == torch.float32:
        return 0
    if fp16 and t.dtype == torch.float16:
        return 2
    raise TypeError(f"unsupported dtype {t.dtype} for this HIP kernel "
                    f"({'bf16/fp16/f32' if fp16 else 'bf16/f32'} only)")


# GPU ops that had to leave the HIP path: (op, reason) -> count. Each (op, reason) warns once;
# tests assert this stays empty on the shapes/dtypes the kernels claim.
FALLBACKS: dict = {}


def fallback(op: str, reason: str) -> None:
    """Record (and warn once about) a GPU op that runs its PyTorch reference instead of HIP."""
    key = (op, reason)
    if key not in FALLBACKS:
        import warnings
        warnings.warn(f"paddle_infer_amd: {op} runs the PyTorch reference on GPU ({reason})",
                      RuntimeWarning, stacklevel=3)
    FALLBACKS[key] = FALLBACKS.get(key, 0) + 1


def main_grad(p):
    """The flat-buffer gradient view of a parameter (set by the training engine), else None."""
    return None if p is None else getattr(p, "main_grad", None)


def fire(p):
    """Signal the engine that ``p``'s gradient is complete (bucketed collective trigger)."""
    hook = getattr(p, "_grad_ready", None)
    if hook is not None:
        hook(p)
