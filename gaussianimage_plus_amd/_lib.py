"""ctypes binding of the C ABI in include/gi2d.h (libgi2d_hip.so, built by csrc/Makefile).

There is deliberately no CPU fallback: if the HIP library is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

# torch bundles its own libamdhip64.so (soname libamdhip64.so.7).  It must be in the process BEFORE
# libgi2d_hip.so is dlopen'ed so that our NEEDED libamdhip64.so.7 binds to that same runtime; loading
# /opt/rocm's copy first would leave two HIP runtimes in one process (hipErrorNoDevice on the second).
import torch  # noqa: F401  (device memory + streams; see module docstring)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# GI2D_LIB: a development variant built by `make VARIANT=...` (csrc/Makefile) instead of the product library -- for the
# measurement scripts under tools/ only; such a library is refused unless GI2D_ALLOW_DEV_BUILD=1 (see load()).
LIB_PATH = os.environ.get("GI2D_LIB") or os.path.join(_HERE, "libgi2d_hip.so")

# include/gi2d.h is the only place the C ABI is written down: every argument list and structure below is read from it
# (_abi.parse), once per process, at the first load() or struct().  csrc/torch_ext/build.py compiles against the same file.
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gi2d.h")
STRUCT_HEADERS = ("gi2d_sample_field.h",)  # next to gi2d.h, which includes them: one structure each, no function

_abi_parsed = None


def abi() -> _abi.Abi:
    global _abi_parsed
    if _abi_parsed is None:
        if not os.path.exists(HEADER_PATH):
            raise RuntimeError(f"{HEADER_PATH} not found: the Python binding reads the C ABI from that header "
                               "(the package runs from a checkout, next to include/).")
        with open(HEADER_PATH) as f:
            parsed = _abi.parse(f.read())
        # the structure headers gi2d.h includes (they declare no function): their structures join the table
        for name in STRUCT_HEADERS:
            with open(os.path.join(os.path.dirname(HEADER_PATH), name)) as f:
                parsed.structs.update(_abi.parse(f.read()).structs)
        _abi_parsed = parsed
    return _abi_parsed


def struct(name: str) -> type:
    """The ctypes.Structure of `struct <name>` in include/gi2d.h (one class per process)."""
    return abi().structs[name]


def __getattr__(name: str):
    """SIGNATURES / SIZE_FUNCS (name -> argtypes of the entries that return a status / a size_t) and STRING_FUNCS (names
    of those that return a string): the parsed header split by return type."""
    kinds = {"SIGNATURES": C.c_int, "SIZE_FUNCS": C.c_size_t, "STRING_FUNCS": C.c_char_p}
    if name not in kinds:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    table = {fn: args for fn, (res, args) in abi().functions.items() if res is kinds[name]}
    return list(table) if name == "STRING_FUNCS" else table


_lib = None


class Gi2dError(RuntimeError):
    """A C-ABI call returned a non-zero status (mirrors the RuntimeError TORCH_CHECK raises)."""


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the gfx950 library has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
            "gaussianimage_plus_amd/csrc`). There is no CPU fallback for this path.")
    functions = abi().functions
    lib = C.CDLL(LIB_PATH)
    lib.gi2d_version.restype, lib.gi2d_version.argtypes = functions["gi2d_version"]
    ver = lib.gi2d_version().decode()  # first: a development build is named before any of its symbols is looked up
    if "dev[" in ver and os.environ.get("GI2D_ALLOW_DEV_BUILD") != "1":
        raise RuntimeError(
            f"{LIB_PATH} is a development build ({ver}): cut-off / knock-out switches give wrong results on purpose. "
            "Rebuild with `make -C gaussianimage_plus_amd/csrc` (no EXTRA), or set GI2D_ALLOW_DEV_BUILD=1 for a "
            "measurement script that knows what it loads.")
    for name, (restype, argtypes) in functions.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.gi2d_last_error_string().decode(errors="replace")
        raise Gi2dError(f"{name} failed (status {rc}): {msg}")


def version() -> str:
    return load().gi2d_version().decode()


class TilePassTimers:
    """`count` kernel timers (gi2d_timer_*) for the tile-pass launches the calling thread issues next: launch
    0, stride, 2 stride, ... carries one (gi2d_timer_arm_many), also inside gi2d_train_steps[_batched] calls.  us() waits
    for the kernels and returns their own execution times -- the figure a rocprofv3 kernel trace reports."""

    def __init__(self, count: int):
        self.handles = []
        for _ in range(int(count)):
            h = C.c_void_p()
            call("gi2d_timer_create", C.byref(h))
            self.handles.append(h)
        self.array = (C.c_void_p * len(self.handles))(*[h.value for h in self.handles])

    def arm(self, stride: int = 1) -> None:
        call("gi2d_timer_arm_many", self.array, len(self.handles), int(stride))

    def cancel(self) -> None:
        call("gi2d_timer_arm_many", None, 0, 1)

    def us(self):
        out = []
        for h in self.handles:
            v = C.c_float()
            call("gi2d_timer_elapsed_us", h, C.byref(v))
            out.append(v.value)
        return out

    def close(self) -> None:
        self.cancel()  # a plan still armed with these handles must not outlive them
        for h in self.handles:
            load().gi2d_timer_destroy(h)
        self.handles = []
