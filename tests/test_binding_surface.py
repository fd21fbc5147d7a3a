"""CPU suite: the Python binding's surface -- names, values, layouts, signatures, docstrings and the ctypes prototypes
of every ABI symbol -- is the one recorded in tests/golden/binding_surface.json.

Run as a script, this module writes that file from the package it loads: do so only on a tree whose binding is the one to
hold later trees to (the snapshot in git was taken before the binding was split into modules)."""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPSHOT = os.path.join(ROOT, "tests", "golden", "binding_surface.json")
#: names with a leading underscore that tests/, tools/ and __graft_entry__.py read from the package
PRIVATE_BUT_READ = ("_lib",)


def _doc(obj):
    d = obj.__doc__
    return None if d is None else hashlib.sha1(" ".join(d.split()).encode()).hexdigest()


def _callable(fn):
    return {"signature": str(inspect.signature(fn)), "doc": _doc(fn)}


def _methods(cls):
    """__init__ and every public method the class answers to, inherited ones included"""
    out = {}
    for name in dir(cls):
        if name.startswith("_") and name != "__init__":
            continue
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, (types.FunctionType, classmethod, staticmethod)):
            out[name] = _callable(getattr(cls, name))
    return out


def _value(name, v):
    if isinstance(v, str) and v.startswith(ROOT):
        v = os.path.relpath(v, ROOT)    # a path into the tree: where the tree lies does not matter
    if name == "LIB_PATH" and os.environ.get("VISO_HIP_LIB"):
        v = "<VISO_HIP_LIB>"            # a child run on another build of the library
    return list(v) if isinstance(v, (tuple, range)) else v


def surface(pkg):
    """what a user of the package can see of it, as plain JSON"""
    pkg_name = pkg.__name__
    names = [n for n in vars(pkg) if not n.startswith("_")] + list(PRIVATE_BUT_READ)
    out = {}
    for name in sorted(names):
        v = getattr(pkg, name)
        if isinstance(v, types.ModuleType):
            if v.__name__.startswith(pkg_name + "."):   # numpy, os and the like are no part of the surface
                out[name] = {"kind": "module"}
        elif type(v).__name__ == "_Feature":             # from __future__ import annotations
            continue
        elif isinstance(v, np.dtype):
            out[name] = {"kind": "dtype", "descr": json.loads(json.dumps(v.descr)), "itemsize": v.itemsize}
        elif isinstance(v, type) and issubclass(v, C.Structure):
            out[name] = {"kind": "structure", "fields": [[f[0], f[1].__name__] for f in v._fields_], "sizeof": C.sizeof(v),
                         "doc": _doc(v), "methods": _methods(v)}
        elif isinstance(v, type):
            out[name] = {"kind": "class", "doc": _doc(v), "methods": _methods(v)}
        elif isinstance(v, types.FunctionType):
            out[name] = {"kind": "function", **_callable(v)}
        else:
            assert isinstance(v, (int, float, str, tuple, range)), (name, type(v))
            out[name] = {"kind": "constant", "type": type(v).__name__, "value": _value(name, v)}
    lib = pkg._lib()
    abi = {}
    for sym in pkg.ABI_SYMBOLS:
        fn = getattr(lib, sym)
        abi[sym] = {"restype": None if fn.restype is None else fn.restype.__name__,
                    "argtypes": None if fn.argtypes is None else [a.__name__ for a in fn.argtypes]}
    return {"names": out, "abi": abi}


def test_binding_surface_is_the_recorded_one(pkg):
    got = json.loads(json.dumps(surface(pkg)))
    want = json.load(open(SNAPSHOT))
    if os.environ.get("VISO_HIP_LIB"):
        want["names"]["LIB_PATH"]["value"] = "<VISO_HIP_LIB>"
    for part in ("names", "abi"):
        assert sorted(got[part]) == sorted(want[part]), (
            part, sorted(set(got[part]) ^ set(want[part])))
        differ = {}
        for k in want[part]:
            g, w = got[part][k], want[part][k]
            if g != w:
                sub = [m for m in set(g.get("methods", {})) | set(w.get("methods", {}))
                       if g.get("methods", {}).get(m) != w.get("methods", {}).get(m)]
                differ[k] = sub or (g, w)
        assert not differ, (part, differ)
    for name in ("Matcher", "StreamGroup", "SequenceGroup", "Reconstruction", "TrackCarry"):
        assert want["names"][name]["methods"], name
    assert len(want["abi"]) == len(pkg.ABI_SYMBOLS)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    with open(SNAPSHOT, "w") as f:
        json.dump(surface(entry.load_package()), f, indent=0, sort_keys=True)
        f.write("\n")
    print(SNAPSHOT, os.path.getsize(SNAPSHOT), "bytes")
