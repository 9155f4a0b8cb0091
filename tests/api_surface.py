"""The public surface of lzma_amd as plain data: every name of dir(lzma_amd) that does not start with "_", and for every
public function, class and method its inspect.signature string and its docstring.  Run as a program it prints that as
JSON, from an interpreter that has imported nothing but the package -- tests/test_api_surface_cpu.py compares the output
with tests/golden/api_surface.json; `python tests/api_surface.py --write` records the fixture anew (only where the
surface is MEANT to change)."""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "api_surface.json")


def _sig(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return None


def _callable(obj):
    return {"kind": "function", "signature": _sig(obj), "doc": obj.__doc__}


def _class(cls):
    """the class's own signature and docstring, and every public attribute it answers to -- wherever in the package's
    classes it is defined: a method that moves into a base class stays part of this surface"""
    members = {}
    for name in dir(cls):
        if name.startswith("_") or any(name in vars(b) for b in cls.__mro__ if b.__module__ == "builtins"):
            continue
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, (staticmethod, classmethod)):
            members[name] = dict(_callable(raw.__func__), kind=type(raw).__name__)
        elif inspect.isfunction(raw):
            members[name] = _callable(raw)
        elif isinstance(raw, property):
            members[name] = {"kind": "property", "doc": raw.__doc__}
        else:
            members[name] = {"kind": "attribute", "value": repr(raw)}
    return {"kind": "class", "signature": _sig(cls), "doc": cls.__doc__, "bases": [b.__name__ for b in cls.__mro__[1:] if not b.__name__.startswith("_")],
            "members": members}


def surface():
    import lzma_amd
    out = {}
    for name in dir(lzma_amd):
        if name.startswith("_"):
            continue
        obj = getattr(lzma_amd, name)
        if inspect.isclass(obj):
            out[name] = _class(obj)
        elif inspect.isfunction(obj):
            out[name] = _callable(obj)
        elif inspect.ismodule(obj):
            out[name] = {"kind": "module", "name": obj.__name__}
        else:
            out[name] = {"kind": "value", "value": repr(obj)}
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    text = json.dumps(surface(), indent=1, sort_keys=True) + "\n"
    assert "torch" not in sys.modules, "importing lzma_amd imported torch"
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
