"""The public surface of the Python binding as text: for every public name of x-slam_amd/pipeline.py and every public attribute of
KinectFusion and ReferenceCallShape its name, inspect.signature (or, for what is not callable, its value) and docstring.
Imported modules are left out.  CPU only; needs the built libraries.  python profiles/tools/pipeline_surface.py | sha256sum"""
import importlib
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pl = importlib.import_module("x-slam_amd.pipeline")


def describe(owner, name):
    v = inspect.getattr_static(owner, name)
    v = v.__func__ if isinstance(v, (staticmethod, classmethod)) else v
    v = v.fget if isinstance(v, property) else v
    if callable(v):
        try:
            what = str(inspect.signature(v))
        except (TypeError, ValueError):
            what = "(no signature)"
        return f"{what}\n    {inspect.getdoc(v)!r}"
    return f"= {v!r}".replace(ROOT, ".") if " at 0x" not in repr(v) else f": {type(v).__name__}"


for n in sorted(vars(pl)):
    if not n.startswith("_") and not inspect.ismodule(getattr(pl, n)):
        print(f"pipeline.{n} {describe(pl, n)}")
for cls in (pl.KinectFusion, pl.ReferenceCallShape):
    for n in sorted(set(dir(cls)) - set(dir(object))):
        if not n.startswith("_"):
            print(f"{cls.__name__}.{n} {describe(cls, n)}")
