"""The max-sum-throughput policy mirrors over worker types that differ
(worker_types=True, max_sum_throughput.py) without a GPU, over the CPU twins
(tests/msttcases.py TwinEngine)."""
import json
import os

import numpy as np
import pytest

import max_sum_throughput as mst
import msttcases as tc

TYPES = ["k80", "p100", "v100"]
COSTS = {"k80": 0.9, "p100": 1.46, "v100": 2.48}


def policy_args(thr, sf, W):
    return ({j: {t: float(thr[j, k]) for k, t in enumerate(TYPES)} for j in range(len(sf))},
            {j: int(sf[j]) for j in range(len(sf))}, {t: int(W[k]) for k, t in enumerate(TYPES)})


@pytest.mark.parametrize("cls,costs", [(mst.ThroughputSumWithPerf, None),
                                        (mst.ThroughputNormalizedByCostSumWithPerf, COSTS),
                                        (mst.ThroughputNormalizedByCostSumWithPerfSLOs, COSTS)])
def test_worker_types_returns_the_kernel_s_vertex(cls, costs):
    W, sf, thr = tc.cases()["zero_type"]
    args = policy_args(thr, sf, W) + (() if costs is None else (costs,))
    with pytest.raises(NotImplementedError, match="the native kernel solves one worker type"):
        cls(native=tc.TwinEngine()).get_allocation(*args)  # unflagged: the recorded text
    eng = tc.TwinEngine()
    pol = cls(native=eng, worker_types=True)
    alloc = pol.get_allocation(*args)
    assert eng.calls == ["mst_allocate_types"]
    x = np.array([[alloc[j][t] for t in TYPES] for j in range(len(sf))])
    w = thr / np.array([1.0 if costs is None else costs[t] for t in TYPES])[None, :]
    want = tc.twin_allocate(W, sf, w)
    assert np.array_equal(x, want[0])
    prices, augs, obj, flags = pol.last_level
    assert np.array_equal(prices, want[1]) and (obj, augs, flags) == (want[2], want[3], want[5])
    assert abs(obj - tc.lp_optimum(W, sf, w)[0]) <= 1e-6 * obj


def test_identical_types_still_go_to_the_one_type_call():
    sf = np.array([1, 2, 4, 1, 2], dtype=np.int32)
    thr = np.repeat(np.array([3.0, 4.0, 5.0, 6.0, 7.0])[:, None], 3, axis=1)
    args = policy_args(thr, sf, [1, 1, 1])
    e0, e1 = tc.TwinEngine(), tc.TwinEngine()
    a0 = mst.ThroughputSumWithPerf(native=e0).get_allocation(*args)
    a1 = mst.ThroughputSumWithPerf(native=e1, worker_types=True).get_allocation(*args)
    assert a0 == a1 and e0.calls == e1.calls == ["mst_allocate"]


def test_refusals_each_followed_by_a_good_call():
    W, sf, thr = tc.cases()["zero_type"]
    pol = mst.ThroughputNormalizedByCostSumWithPerfSLOs(native=tc.TwinEngine(), worker_types=True)
    good = policy_args(thr, sf, W) + (COSTS,)
    want = pol.get_allocation(*good)
    with pytest.raises(NotImplementedError, match="SLOs and throughputs or instance costs that differ"):
        pol.get_allocation(*good, SLOs={0: 100.0}, num_steps_remaining={0: 10})
    assert pol.get_allocation(*good) == want
    with pytest.raises(ValueError, match="worker type p100"):
        pol.get_allocation(*good[:3], dict(COSTS, p100=0.0))
    assert pol.get_allocation(*good) == want
    assert pol.get_allocation({}, {}, {t: 1 for t in TYPES}) is None
    # the unflagged text is the one the golden file records
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "policy_mirrors.json")))
    with pytest.raises(NotImplementedError) as e:
        mst.ThroughputSumWithPerf(native=tc.TwinEngine()).get_allocation(*good[:3])
    assert str(e.value) in json.dumps(golden, ensure_ascii=False)
