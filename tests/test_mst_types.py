"""Max sum throughput over worker types that differ (csrc/sw_mst_types.h) without
a GPU: the CPU twin (tests/twins/mstt_twin.c) against its own optimality
certificate and against the reference's LP through HiGHS, at the shapes of
tests/msttcases.py."""
import numpy as np
import pytest

import msttcases as tc

SMALL = [n for n in tc.cases() if not n.startswith("lds")]


@pytest.mark.parametrize("name", list(tc.cases()))
def test_certificate(name):
    """Integer feasibility, and weak duality closed from the returned prices:
    |D(prices) − objective| ≤ 4·m·n·ε·objective, the rounding of the m·n terms of
    either sum (ε = 2^-53).  Largest gap measured: 1.9 ε (lds_limit), 0 on most."""
    W, sf, w = tc.cases()[name]
    out = tc.twin_of(name)
    gap = tc.certificate(W, sf, w, out)
    print(f"{name}: gap {gap / tc.EPS:.1f} eps, {out[3]} augmentations on {len(sf)} jobs, {out[4]} rows")
    assert gap <= 4 * w.size * tc.EPS
    assert len(sf) <= out[3] <= tc.const("cap_mult") * (len(sf) + len(W))


@pytest.mark.parametrize("name", SMALL)
def test_against_highs(name):
    """The objective at 1e-6 relative (measured ≤ 4.1e-16).  On the continuous
    random weights (every case but ties) the optimum is unique and the shares are
    HiGHS's vertex: worst difference measured 0.0, so the bar is 1e-12, the
    solver's own feasibility tolerance of 1e-9 on shares of size ≤ 1 apart."""
    W, sf, w = tc.cases()[name]
    x, _, obj = tc.twin_of(name)[:3]
    ref_obj, ref_x = tc.lp_optimum(W, sf, w)
    print(f"{name}: objective rel {abs(obj - ref_obj) / ref_obj:.1e}, shares {np.abs(x - ref_x).max():.1e}")
    assert abs(obj - ref_obj) <= 1e-6 * ref_obj
    if name != "ties":
        assert np.abs(x - ref_x).max() <= 1e-12


def test_shapes_take_the_paths_they_were_built_for():
    import mst_ref

    W, sf, w = tc.cases()["n1"]  # one type: the objective of the one-type kernel
    assert tc.twin_of("n1")[2] == pytest.approx(mst_ref.twin_allocate(sf, w[:, 0], None, int(W[0]))[3], rel=1e-12)
    x, prices, obj, augs, rows, flags = tc.twin_of("chain4")
    assert np.array_equal(x, np.roll(np.eye(4), 1, axis=1)) and (obj, augs, flags) == (22.0, 4, 0)
    assert list(prices) == [10.0, 4.0, 3.0, 2.0]
    assert (tc.twin_of("zero_type")[0][:, 1] == 0.0).all()
    x = tc.twin_of("wide")[0]  # every job wider than every type: capacity is all used, in quarters
    assert np.array_equal((x * 4).sum(axis=0), [2, 3, 1]) and tc.twin_of("wide")[5] == tc.const("flag_unplaced")
    x, prices, *_, flags = tc.twin_of("roomy")
    assert flags == tc.const("flag_slack") and (prices == 0.0).all() and (x.sum(axis=1) == 1.0).all()
    # exact ties: the lowest job keeps the contested type
    x = tc.twin_allocate([1], [1, 1], [[3.0], [3.0]])[0]
    assert x.tolist() == [[1.0], [0.0]]
    x = tc.twin_allocate([1, 1], [1], [[2.0, 2.0]])[0]  # and the lowest type
    assert x.tolist() == [[1.0, 0.0]]
