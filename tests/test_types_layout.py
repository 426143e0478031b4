"""csrc/sw_types_layout.h on the host: the arithmetic of the worker-type frame
(tests/native/types_layout_check.cpp).

The program checks, for the column sets of the four worker-type policies, that
the views of the input and output blocks are aligned and tile them, that every
offset equals the formula the policy's call held before the frame and the
padded input size that formula's end rounded up to 8, that packing and
unpacking reproduce the arrays (the results without their status word), and
the common rejections with their texts and order.  It is built twice — plain,
and with the address and undefined-behaviour sanitizers — as a stand-alone host
program that includes that header only.
"""
from nativecheck import CSRC, SANITIZE, build_and_run

SRC = "types_layout_check.cpp"  # in tests/native/
FLAGS = ["-I", CSRC]


def test_types_layout_properties(tmp_path):
    assert build_and_run(tmp_path, SRC, "types_layout_check", "c++", FLAGS) > 3000


def test_types_layout_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "types_layout_check_san", "c++", FLAGS + SANITIZE)
    assert checks > 3000
