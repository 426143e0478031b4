"""csrc/sw_alloc_layout.h on the host: the arithmetic of the allocation frame
(tests/native/alloc_layout_check.cpp).

The program checks, for column sets shaped like those of the four per-job
policies, that the views of the input and output blocks are aligned and tile
them, that the block sizes equal each policy's formula, that packing and
unpacking reproduce the columns (an absent one as zeros), the LDS staging
bound maxq around 512 and LDS_JOBS with its environment switch, and the
rejections of bad offsets and worker counts with their texts and order.  It is
built twice — plain, and with the address and undefined-behaviour sanitizers —
as a stand-alone host program that includes that header only.
"""
from nativecheck import CSRC, SANITIZE, build_and_run

SRC = "alloc_layout_check.cpp"  # in tests/native/
FLAGS = ["-I", CSRC]


def test_alloc_layout_properties(tmp_path):
    assert build_and_run(tmp_path, SRC, "alloc_layout_check", "c++", FLAGS) > 700


def test_alloc_layout_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "alloc_layout_check_san", "c++", FLAGS + SANITIZE)
    assert checks > 700
