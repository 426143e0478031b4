"""TEST INFRASTRUCTURE: the shared libraries the tests reach through ctypes —
the CPU twins built by csrc/Makefile into shockwave-replication_amd/lib/, the
plan twin built by oracle/Makefile into oracle/_build/, and the probe libraries
of the device code.  Only tests/ (and tools/ run by hand) may import this module.
"""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")
LIB = os.path.join(ROOT, "shockwave-replication_amd", "lib")
ORACLE = os.path.join(ROOT, "oracle")
_LOADED = {}


def load(so_name, declare, built_by=None):
    """The library, loaded once per declare function, which sets the argtypes
    and restypes of what its module calls.  An absent library is made first:
    by csrc/Makefile (built_by="csrc", into lib/) or by oracle/Makefile
    (built_by="oracle", into oracle/_build/, or wherever SW_TWIN_PATH names).
    With built_by=None (a probe library of the device code in lib/) an absent
    library means the build is broken: there is no fall-back."""
    if (so_name, declare) not in _LOADED:
        if built_by == "oracle":
            path = os.environ.get("SW_TWIN_PATH") or os.path.join(ORACLE, "_build", so_name)
            make = ["make", "-s", "-C", ORACLE]
        else:
            path = os.path.join(LIB, so_name)
            make = ["make", "-s", "-C", CSRC, "../lib/" + so_name]
        if built_by is not None and not os.path.exists(path):
            subprocess.check_call(make)
        lib = ctypes.CDLL(path)
        declare(lib)
        _LOADED[so_name, declare] = lib
    return _LOADED[so_name, declare]
