"""ctypes binding of libmgunet.so.  The prototypes are read from include/mgunet.h itself; `call` is the one path from the modules
to an entry point: no torch types cross the boundary, only device pointers (tensor.data_ptr()), sizes and the HIP stream handle.
There is no CPU fallback: if the shared library is missing or no HIP device exists, every call raises."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)                      # .../mingraph-unet_amd
CSRC = os.path.join(PKG_ROOT, "csrc")
# MGU_LIB_PATH: developer hook for A/B runs of two builds of the SAME sources tree (tools/gpu_r03_ab.sh); the default is the in-tree build
LIB_PATH = os.environ.get("MGU_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libmgunet.so")

MGU_OK, MGU_ERR_INVALID, MGU_ERR_HIP, MGU_ERR_STATE, MGU_ERR_NOMEM = 0, -1, -2, -3, -4


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ptr", C.c_void_p), ("numel", C.c_int64)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("flops_alg", C.c_double), ("flops_mfma", C.c_double),
                ("launches", C.c_int), ("pipe", C.c_int)]


class OptimDesc(C.Structure):
    """mgu_optim_desc (include/mgunet.h): the options of one mgu_optim_step."""
    _fields_ = [("kind", C.c_int), ("lr", C.c_float), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("momentum", C.c_float), ("grad_scale", C.c_float), ("max_norm", C.c_float),
                ("skip_nonfinite", C.c_int), ("ema_decay", C.c_float), ("ema_warmup", C.c_int)]


OPTIM_KINDS = {"adam": 0, "adamw": 1, "sgd": 2}     # MGU_OPTIM_*
OPTIM_CTRL_BYTES = 64                               # MGU_OPTIM_CTRL_BYTES


def read_kernel_stats(ctx) -> list:
    """mgu_profile_read_kernels as a list of dicts (per kernel family since mgu_profile_enable(ctx, 1))."""
    arr = (KernelStat * 64)()
    n = C.c_int()
    check(lib().mgu_profile_read_kernels(ctx.handle, arr, 64, C.byref(n)), ctx.handle)
    return [{"name": arr[i].name.decode(), "ms": arr[i].ms, "flops_alg": arr[i].flops_alg, "flops_mfma": arr[i].flops_mfma,
             "launches": arr[i].launches, "pipe": arr[i].pipe} for i in range(n.value)]


_lib = None
_lock = threading.Lock()

HEADER = os.path.join(os.path.dirname(PKG_ROOT), "include", "mgunet.h")
_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "unsigned long long": C.c_uint64, "float": C.c_float,
           "double": C.c_double, "size_t": C.c_size_t, "void": None, "char*": C.c_char_p, "mgu_tensor_desc*": C.POINTER(TensorDesc)}


def _ctype(t: str, decl: str):
    t = re.sub(r"\s*\*", "*", " ".join(re.sub(r"\bconst\b", "", t).split()))   # "void* const*" -> "void**"
    if t in _CTYPES:
        return _CTYPES[t]
    if t.endswith("*"):                                                   # every other pointer, host or device
        return C.c_void_p
    raise TypeError(f"mgunet.h: no ctypes type for '{t}' in `{decl}`")


def parse_header(path: str = HEADER) -> dict:
    """name -> (restype, argtypes, takes_stream) of every `ret mgu_name(params);` the header declares; takes_stream: the last
    parameter is `hip_stream`."""
    txt = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", "", open(path).read(), flags=re.S | re.M)
    protos = {}
    for m in re.finditer(r"([\w\s*]+?)\b(mgu_\w+)\s*\(([^)]*)\)\s*;", txt):
        ret, name, params = m.groups()
        decl = " ".join(m.group(0).split())
        ps = [re.fullmatch(r"(.+?)\s*\b(\w+)", p.strip()) for p in params.split(",")] if params.strip() not in ("", "void") else []
        if not all(ps):
            raise TypeError(f"mgunet.h: unnamed parameter in `{decl}`")
        protos[name] = (_ctype(ret, decl), [_ctype(p[1], decl) for p in ps], bool(ps) and ps[-1][2] == "hip_stream")
    return protos


_PROTOS = {}   # parse_header(), installed by lib()
_CALLS = {}    # name -> (function, takes_stream)


def build(verbose: bool = False) -> str:
    """Compile csrc/ for gfx950 into lib/libmgunet.so (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode:
        raise RuntimeError("building libmgunet.so failed (see output above)")
    return LIB_PATH


def lib() -> C.CDLL:
    """Load (once) and return the shared library with prototypes installed."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(or `make -C mingraph-unet_amd/csrc`).  There is no CPU fallback.")
            L = C.CDLL(LIB_PATH)
            _PROTOS.update(parse_header())
            for name, (res, args, takes_stream) in _PROTOS.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
                _CALLS[name] = (fn, takes_stream)
            _lib = L
    return _lib


def check(rc: int, ctx=None) -> None:
    """Map a C-ABI return code to the exception type the reference's Python would raise."""
    if rc == MGU_OK:
        return
    msg = lib().mgu_last_error(ctx)
    msg = msg.decode() if msg else f"libmgunet error {rc}"
    if rc == MGU_ERR_INVALID:
        raise ValueError(msg)
    if rc == MGU_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


class Context:
    """One mgu_ctx per (object, device)."""

    def __init__(self, device_index: int):
        self.handle = C.c_void_p()
        self.device_index = device_index
        check(lib().mgu_create(device_index, C.byref(self.handle)), None)

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                lib().mgu_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass


_CTX = {}


def context(device: torch.device) -> Context:
    """The Context shared by everything on `device` that does not configure one of its own (the UNet does)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ctx = _CTX.get(idx)
    if ctx is None:
        ctx = _CTX[idx] = Context(idx)
    return ctx


def current_stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def call(name: str, device, *args, ctx: Context = None) -> None:
    """Run the status-returning entry point `name` on `device` (the device of `ctx` when one is given) and raise on failure.  The
    context (the shared one unless `ctx` is given) goes first, a tensor argument as its data_ptr(), the device's current stream
    last where the prototype ends in `hip_stream`.  device=None: a host routine, which takes neither a context nor a stream."""
    if _lib is None:
        lib()
    fn, takes_stream = _CALLS[name]
    if device is None:
        check(fn(*args))
        return
    if ctx is None:
        ctx = context(device)
    idx = ctx.device_index
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(idx):
        if takes_stream:
            args.append(torch.cuda.current_stream(idx).cuda_stream)
        check(fn(ctx.handle, *args), ctx.handle)


def require_hip(t, what: str) -> None:
    """Raise unless the tensor (or torch.device) `t` is on a HIP device."""
    if (t if isinstance(t, torch.device) else t.device).type != "cuda":
        raise RuntimeError(f"{what} runs only on a HIP device (MI355X); there is deliberately no CPU fallback")


class Prepared:
    """A prepared-weights handle (mgu_gat_prepare / mgu_conv2d_prepare: `prepare(..., &out, hip_stream)`), released with the object.
    `key` records what it was prepared from."""

    def __init__(self, prepare: str, device, *args, ctx: Context = None, key=None):
        self.ctx = ctx if ctx is not None else context(device)
        self.release, self.key, self.handle = prepare.replace("_prepare", "_release"), key, C.c_void_p()
        call(prepare, device, *args, C.byref(self.handle), ctx=self.ctx)

    def __del__(self):
        try:
            if self.handle:
                getattr(lib(), self.release)(self.ctx.handle, self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass
