"""Every refusal the host tests of the terrain calls provoke, as text: one line per refused call with the test, the entry
point, the return code and the whole of mrtx_last_error.  Run it once per library and compare the files: a refactor of the host
units must leave them identical byte for byte.  Needs no GPU.

    python tools/refusal_texts.py before.txt --lib /path/to/the/parent/libmoonrt.so
    python tools/refusal_texts.py after.txt
    cmp before.txt after.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ["test_illumination_host", "test_illum_series_host", "test_horizon_host", "test_mast_host", "test_timed_traverse_host",
           "test_power_host", "test_sight_host", "test_thermal_host", "test_scatter_host", "test_volatiles_host",
           "test_traverse_host", "test_relief_host", "test_terrain_host"]


class Recorder:
    """A pytest plugin: every mrtx_* call that returns a code other than MRTX_OK is written down under the running test."""

    def __init__(self, lib, signatures, ctx_type):
        self.lines, self.test = [], "?"
        for name, (res, args) in signatures.items():
            if res is not None and name not in ("mrtx_abi_version", "mrtx_create", "mrtx_last_error"):
                setattr(lib, name, self.wrap(lib, name, getattr(lib, name), bool(args) and args[0] is ctx_type))

    def wrap(self, lib, name, fn, has_ctx):
        def call(*a):
            rc = fn(*a)
            if isinstance(rc, int) and rc != 0:
                ctx = a[0] if has_ctx and a else None
                text = lib.mrtx_last_error(ctx).decode(errors="replace") if ctx else "(no context)"
                self.lines.append(f"{self.test}\t{name}\t{rc}\t{text}")
            return rc
        call.argtypes, call.restype = fn.argtypes, fn.restype       # what a test may ask the function itself
        return call

    def pytest_runtest_setup(self, item):
        self.test = item.nodeid


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", help="the file to write")
    ap.add_argument("--lib", help="the library to load instead of the tree's own (MOONRT_LIB)")
    args = ap.parse_args()
    if args.lib:
        os.environ["MOONRT_LIB"] = os.path.abspath(args.lib)
    sys.path.insert(0, ROOT)
    import pytest
    from moonrtx_amd import _lib
    lib = _lib.load()
    rec = Recorder(lib, _lib.SIGNATURES, _lib._VP)
    rc = pytest.main(["-q", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", m + ".py") for m in MODULES], plugins=[rec])
    with open(args.out, "w") as f:
        f.write("\n".join(rec.lines) + "\n")
    print(f"{len(rec.lines)} refused calls of {_lib.LIB_PATH} written to {args.out}; pytest's exit code {int(rc)}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
