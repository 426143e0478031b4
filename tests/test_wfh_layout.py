"""csrc/sw_wfh_layout.h on the host: the checks, the block layout and the
member-order packing of a hierarchical water-filling call
(tests/native/wfh_layout_check.cpp), built twice — plain, and with the address
and undefined-behaviour sanitizers — as a stand-alone host program that
includes that header only."""
from nativecheck import CSRC, SANITIZE, build_and_run

SRC = "wfh_layout_check.cpp"  # in tests/native/
FLAGS = ["-I", CSRC]


def test_wfh_layout_properties(tmp_path):
    assert build_and_run(tmp_path, SRC, "wfh_layout_check", "c++", FLAGS) > 5000


def test_wfh_layout_under_sanitizers(tmp_path):
    checks = build_and_run(tmp_path, SRC, "wfh_layout_check_san", "c++", FLAGS + SANITIZE)
    assert checks > 5000
