"""ctypes binding of libsde.so (the C ABI declared in include/sde.h).

torch is imported first on purpose: its bundled HIP runtime (SONAME
libamdhip64.so.7) is then the one libsde.so binds to, so device pointers and
streams handed over from torch are valid in our launches.

There is no fallback: if the library is missing or does not export a symbol of
include/sde.h, importing this module raises.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (load torch's HIP runtime before libsde.so)

from ._build import INCLUDE, LIB

HEADER = os.path.join(INCLUDE, "sde.h")

# every scalar type include/sde.h may use; any pointer is a c_void_p.  A type outside this map is an error
# (parse_header raises), never a guess: a wrong width is a silent miscall.
CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64,
          "float": ctypes.c_float, "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"([\w\s\*]+?)\b(sde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_NUMBER = re.compile(r"(-?\d+)|(-?\d+\.\d*(?:[eE][-+]?\d+)?)f?")


def _strip_comments(text: str) -> str:
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _ctype(decl: str, name: str, returns: bool = False):
    """The ctypes type of one declaration (`const float *fl`, `int64_t npix`, a bare return type)."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if returns and words[:-1] == ["const", "char"] else ctypes.c_void_p
    base = [w for w in (words if returns else words[:-1]) if w != "const"]
    if len(base) != 1 or base[0] not in CTYPES:
        raise TypeError(f"include/sde.h: {name}: no ctypes mapping for `{decl.strip()}`")
    return CTYPES[base[0]]


def parse_header(text: str):
    """Header text -> ({function: (restype, argtypes)}, {SDE_* constant: number}): the binding's only source.
    Constants are the `#define SDE_X number` lines (an `f` suffix dropped) and the members of every enum."""
    text = _strip_comments(text)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SDE_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        m = _NUMBER.fullmatch(value)
        if not m:
            raise TypeError(f"include/sde.h: #define {name} {value}: not a number")
        constants[name] = int(m.group(1)) if m.group(1) else float(m.group(2))
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        for member in filter(None, (t.strip() for t in body.split(","))):
            m = re.fullmatch(r"(SDE_\w+)\s*=\s*(-?\d+)", member)
            if not m:
                raise TypeError(f"include/sde.h: enum member `{member}`: expected SDE_NAME = integer")
            constants[m.group(1)] = int(m.group(2))
    signatures = {}
    for ret, name, params in _PROTOTYPE.findall(re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (_ctype(ret, name, returns=True), [_ctype(p, name) for p in params])
    return signatures, constants


def header_functions(path: str = HEADER):
    """Names of the functions declared in include/sde.h, by a looser rule than parse_header's (any `sde_name(`
    outside a comment): tests hold the two against each other, so a prototype the parser skips is noticed."""
    with open(path) as fh:
        return sorted(set(re.findall(r"\b(sde_[a-z0-9_]+)\s*\(", _strip_comments(fh.read()))))


with open(HEADER) as _fh:
    SIGNATURES, CONSTANTS = parse_header(_fh.read())   # name -> (restype, argtypes); SDE_* name -> number
globals().update(CONSTANTS)   # _lib.SDE_LAYOUT_DHW, ... as module attributes


class SdeError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB):
        raise ImportError(f"{LIB} is missing: build it with `python -m scenedepthestimation_amd._build` "
                          "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB)
    missing = []
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise ImportError(f"{LIB} does not export {missing}")
    # a library of another ABI would take these argument lists with other meanings (e.g. ABI 3 added
    # the aggregation workspace): refuse it rather than pass it the wrong arguments
    abi = CONSTANTS["SDE_ABI_VERSION"]
    if lib.sde_abi_version() != abi:
        raise ImportError(f"{LIB} has ABI {lib.sde_abi_version()}, this binding needs {abi}: rebuild it")
    return lib


lib = _load()


def check(status: int, what: str):
    if status != CONSTANTS["SDE_OK"]:
        msg = lib.sde_status_string(status)
        raise SdeError(f"{what} failed: {msg.decode() if msg else status} ({status})")
