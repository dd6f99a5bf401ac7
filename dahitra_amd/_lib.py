"""ctypes binding of libdahitra_hip.so (C ABI: include/dahitra_hip.h).

The header drives the binding: lib() gives every declared function the restype and argtypes of its own prototype, so callers
pass plain Python numbers and ctypes refuses a call that lacks an argument or passes a scalar of the wrong kind.  A new entry
point needs its declaration in the header and nothing here.

The library is the product's only arithmetic path.  There is no CPU / eager fallback: if the
shared object is missing or a call fails, a RuntimeError is raised."""
import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# DAHITRA_HIP_LIB: an experiment build of the same library (tools/*_timeline.py); the product path is the in-tree one
LIB_PATH = os.environ.get("DAHITRA_HIP_LIB") or os.path.join(_HERE, "lib", "libdahitra_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dahitra_hip.h")

_lib = None


class HipLibraryError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "char*": ctypes.c_char_p})


def _ctype(decl, table, pointer=None):
    """`decl`: a C type, `const` ignored.  A type `table` does not name is `pointer` if it is one; nothing is guessed."""
    key = re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\bconst\b", " ", decl).split()))
    if key in table:
        return table[key]
    if pointer is None or not re.fullmatch(r"[a-z ]+\*+", key):
        raise ValueError("dahitra_hip.h: unknown type %r" % decl.strip())
    return pointer


def parse_prototypes(text):
    """C declarations of dh_* functions -> {name: (restype, [argtypes])} in ctypes terms"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(dh_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(.*?[\s*])([A-Za-z_]\w*)\s*", p, flags=re.S)       # type, then the parameter's name
            if m is None:
                raise ValueError("dahitra_hip.h: %s: cannot read the parameter %r" % (name, p.strip()))
            args.append(_ctype(m.group(1), _SCALARS, ctypes.c_void_p))
        protos[name] = (_ctype(ret, _RETURNS), args)
    unread = sorted(set(re.findall(r"\b(dh_[a-z0-9_]+)\s*\(", text)) - set(protos))
    if unread:
        raise ValueError("dahitra_hip.h: cannot read the declaration of %s" % ", ".join(unread))
    return protos


@functools.lru_cache(None)
def prototypes():
    """{name: (restype, [argtypes])} of every dh_* function declared in include/dahitra_hip.h (parsed once per process)"""
    return parse_prototypes(open(HEADER_PATH).read())


def declared_symbols():
    """Every dh_* function declared in include/dahitra_hip.h."""
    return sorted(prototypes())


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError("dahitra_amd: %s not found -- build it with `make` (or __graft_entry__.build()); "
                                  "there is no fallback path" % LIB_PATH)
        dll = ctypes.CDLL(LIB_PATH)
        missing = [name for name in prototypes() if not hasattr(dll, name)]
        if missing:
            raise HipLibraryError("dahitra_amd: %s lacks symbols declared in include/dahitra_hip.h: %s" % (LIB_PATH, missing))
        for name, (restype, argtypes) in prototypes().items():
            fn = getattr(dll, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = dll
    return _lib


def check(rc, what):
    if rc != 0:
        raise HipLibraryError("%s failed: %s" % (what, lib().dh_last_error().decode()))
