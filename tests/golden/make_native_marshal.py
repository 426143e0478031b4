"""Generate tests/golden/native_marshal.json: the signatures sw_native.load()
declares and, for every scenario of tests/test_native_marshal.py, what the
binding hands to a recording stand-in for the C library and what it returns or
raises (no GPU).  Every float is stored as ``float.hex``.

    python tests/golden/make_native_marshal.py

Run it at the commit whose behaviour is to be pinned, after a build
(``load()`` reads the signatures off the built library).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the product directory on the path)
import test_native_marshal as tnm  # noqa: E402

OUT = os.path.join(HERE, "native_marshal.json")


def main():
    rec = tnm.record()
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_native_marshal.py", **rec}, f, separators=(",", ":"),
                  sort_keys=True)
        f.write("\n")
    calls = sum(len(r["calls"]) for r in rec["scenarios"].values())
    print(f"wrote {OUT}: {len(rec['signatures'])} signatures, {len(rec['scenarios'])} scenarios, {calls} calls, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
