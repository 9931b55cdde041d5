"""ctypes binding of libsde.so (the C ABI declared in include/sde.h, the geometry stage's in include/sde_geom.h,
the filters' in include/sde_filter.h, the uniqueness check's in include/sde_unique.h and the interpolation's in
include/sde_interp.h).

torch is imported first on purpose: its bundled HIP runtime (SONAME
libamdhip64.so.7) is then the one libsde.so binds to, so device pointers and
streams handed over from torch are valid in our launches.

There is no fallback: if the library is missing or does not export a symbol of
any header, importing this module raises.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch  # noqa: F401  (load torch's HIP runtime before libsde.so)

from ._build import INCLUDE, LIB

# function prefix -> the header that declares it; constants carry the prefix in capitals (SDE_*, SDG_*, SDF_*, SDU_*,
# SDI_*)
HEADER_NAMES = {"sde": "sde.h", "sdg": "sde_geom.h", "sdf": "sde_filter.h", "sdu": "sde_unique.h",
                "sdi": "sde_interp.h"}
HEADER = os.path.join(INCLUDE, HEADER_NAMES["sde"])
GEOM_HEADER = os.path.join(INCLUDE, HEADER_NAMES["sdg"])
FILTER_HEADER = os.path.join(INCLUDE, HEADER_NAMES["sdf"])
UNIQUE_HEADER = os.path.join(INCLUDE, HEADER_NAMES["sdu"])
INTERP_HEADER = os.path.join(INCLUDE, HEADER_NAMES["sdi"])

# every scalar type the headers may use; any pointer is a c_void_p.  A type outside this map is an error
# (parse_header raises), never a guess: a wrong width is a silent miscall.
CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64,
          "float": ctypes.c_float, "double": ctypes.c_double}
_NUMBER = re.compile(r"(-?\d+)|(-?\d+\.\d*(?:[eE][-+]?\d+)?)f?")


def _strip_comments(text: str) -> str:
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _ctype(decl: str, name: str, returns: bool = False, header: str = "include/sde.h"):
    """The ctypes type of one declaration (`const float *fl`, `int64_t npix`, a bare return type)."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if returns and words[:-1] == ["const", "char"] else ctypes.c_void_p
    base = [w for w in (words if returns else words[:-1]) if w != "const"]
    if len(base) != 1 or base[0] not in CTYPES:
        raise TypeError(f"{header}: {name}: no ctypes mapping for `{decl.strip()}`")
    return CTYPES[base[0]]


def parse_header(text: str, prefix: str = "sde"):
    """Header text -> ({function: (restype, argtypes)}, {constant: number}) for the functions `prefix`_name and
    the constants PREFIX_NAME: the binding's only source.  Constants are the `#define PREFIX_X number` lines (an
    `f` suffix dropped) and the members of every enum; `#define`s and prototypes of another prefix are passed
    over."""
    text = _strip_comments(text)
    hdr, cap = "include/" + HEADER_NAMES[prefix], prefix.upper()
    constants = {}
    for name, value in re.findall(rf"^[ \t]*#[ \t]*define[ \t]+({cap}_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        m = _NUMBER.fullmatch(value)
        if not m:
            raise TypeError(f"{hdr}: #define {name} {value}: not a number")
        constants[name] = int(m.group(1)) if m.group(1) else float(m.group(2))
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        for member in filter(None, (t.strip() for t in body.split(","))):
            m = re.fullmatch(rf"({cap}_\w+)\s*=\s*(-?\d+)", member)
            if not m:
                raise TypeError(f"{hdr}: enum member `{member}`: expected {cap}_NAME = integer")
            constants[m.group(1)] = int(m.group(2))
    signatures = {}
    prototype = re.compile(rf"([\w\s\*]+?)\b({prefix}_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
    for ret, name, params in prototype.findall(re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (_ctype(ret, name, True, hdr), [_ctype(p, name, False, hdr) for p in params])
    return signatures, constants


def header_functions(path: str = None, prefix: str = "sde"):
    """Names of the functions `prefix`_name declared in a header (default: the header of that prefix), by a looser
    rule than parse_header's (any `prefix_name(` outside a comment): tests hold the two against each other, so a
    prototype the parser skips is noticed."""
    if path is None:
        path = os.path.join(INCLUDE, HEADER_NAMES[prefix])
    with open(path) as fh:
        return sorted(set(re.findall(rf"\b({prefix}_[a-z0-9_]+)\s*\(", _strip_comments(fh.read()))))


with open(HEADER) as _fh:
    SIGNATURES, CONSTANTS = parse_header(_fh.read())   # name -> (restype, argtypes); SDE_* name -> number
with open(GEOM_HEADER) as _fh:
    GEOM_SIGNATURES, GEOM_CONSTANTS = parse_header(_fh.read(), prefix="sdg")   # the same, sdg_* / SDG_*
with open(FILTER_HEADER) as _fh:
    FILTER_SIGNATURES, FILTER_CONSTANTS = parse_header(_fh.read(), prefix="sdf")   # sdf_* / SDF_*
with open(UNIQUE_HEADER) as _fh:
    UNIQUE_SIGNATURES, UNIQUE_CONSTANTS = parse_header(_fh.read(), prefix="sdu")   # sdu_* / SDU_*
with open(INTERP_HEADER) as _fh:
    INTERP_SIGNATURES, INTERP_CONSTANTS = parse_header(_fh.read(), prefix="sdi")   # sdi_* / SDI_*
globals().update(CONSTANTS)   # _lib.SDE_LAYOUT_DHW, ... as module attributes
globals().update(GEOM_CONSTANTS)
globals().update(FILTER_CONSTANTS)
globals().update(UNIQUE_CONSTANTS)
globals().update(INTERP_CONSTANTS)


class SdeError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB):
        raise ImportError(f"{LIB} is missing: build it with `python -m scenedepthestimation_amd._build` "
                          "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB)
    missing = []
    for name, (res, args) in {**SIGNATURES, **GEOM_SIGNATURES, **FILTER_SIGNATURES, **UNIQUE_SIGNATURES,
                              **INTERP_SIGNATURES}.items():
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
