"""TEST INFRASTRUCTURE: the stand-alone host programs of tests/native/ — built
with the host compiler, run, and their ``ok <checks>`` line read.  Nothing is
loaded into Python.  Only tests/ may import this module.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shockwave-replication_amd", "csrc")
# language → compiler, the flags every check of that language has, what follows the source
_LANG = {"c": ("gcc", ["-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function"], ["-lm"]),
         "c++": ("g++", ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"], [])}
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            # the runtimes inside the program: it must start whatever else the
            # environment loads into it first
            "-static-libasan", "-static-libubsan"]


def build_and_run(tmp_path, src, name, lang, extra=(), args=(), timeout=120):
    """Build tests/native/<src> as tmp_path/<name> with the flags of lang ("c"
    or "c++") and extra, run it on args, and return the number of checks it
    reports."""
    compiler, flags, libs = _LANG[lang]
    cc = shutil.which(compiler)
    assert cc, f"no host {lang.upper()} compiler ({compiler})"
    exe = str(tmp_path / name)
    subprocess.check_call([cc, *flags, *extra, "-o", exe, os.path.join(ROOT, "tests", "native", src), *libs])
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout + r.stderr
    return int(r.stdout.split()[1])
