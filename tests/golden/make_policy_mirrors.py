"""Generate tests/golden/policy_mirrors.json: what every public policy class of
the seven host mirrors returns, keeps in its ``last_*`` attributes, warns and
raises on the inputs of tests/test_policy_mirrors.py, computed with the CPU
twins (no GPU).  Every float is stored as ``float.hex``.

    python tests/golden/make_policy_mirrors.py

Run it at the commit whose behaviour is to be pinned, after a build (the twins
are shared libraries under shockwave-replication_amd/lib/).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the product directory and oracle/ on the path)
import test_policy_mirrors as tpm  # noqa: E402

OUT = os.path.join(HERE, "policy_mirrors.json")


def main():
    classes = tpm.record()
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_policy_mirrors.py", "classes": classes}, f, separators=(",", ":"),
                  sort_keys=True)
        f.write("\n")
    calls = sum(len(c) for s in classes.values() for c in s.values())
    print(f"wrote {OUT}: {len(classes)} classes, {calls} calls, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
