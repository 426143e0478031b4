"""The policy mirror of the hierarchical water filling
(max_min_fairness_water_filling_hierarchical.py) on the CPU twin engine: the
reference's signatures, its errors, several identical worker types, and an
instance of the shape of the reference's water_filling_tests_hierarchical.py."""
import inspect
import math

import numpy as np
import pytest

import max_min_fairness_water_filling as wf
import max_min_fairness_water_filling_hierarchical as wfh
import wfh_ref
import wfhcases as wc

CLASSES = (wfh.MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf, wfh.MaxMinFairnessWaterFillingHierarchicalPolicy)


def small(tp=None):
    """Two entities over five jobs on 5 workers: team a (fairness, weight 2)
    holds jobs 0 and 3, team b (fifo, weight 3) jobs 1, 2 and 4."""
    tp = tp or {j: {"v100": 2.0 + j} for j in range(5)}
    return dict(throughputs=tp, scale_factors={0: 2, 1: 1, 2: 1, 3: 1, 4: 1},
                priority_weights={0: 2.0, 1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0}, cluster_spec={"v100": 5},
                entity_weights={"a": 2.0, "b": 3.0}, entity_to_job_mapping={"a": [0, 3], "b": [4, 1, 2]},
                policies={"a": "fairness", "b": "fifo"})


def test_signatures_are_the_references():
    for cls in CLASSES:
        assert list(inspect.signature(cls.__init__).parameters)[:2] == ["self", "priority_reweighting_policies"]
        assert list(inspect.signature(cls.get_allocation).parameters) == [
            "self", "unflattened_throughputs", "scale_factors", "unflattened_priority_weights", "cluster_spec",
            "entity_weights", "entity_to_job_mapping", "verbose", "return_effective_throughputs"]
        assert (inspect.signature(cls.get_allocation).parameters.keys()
                == inspect.signature(wf.MaxMinFairnessWaterFillingPolicy.get_allocation).parameters.keys())
    assert CLASSES[0]({"a": "fifo"}).name == "MaxMinFairnessWaterFilling_Perf"
    assert CLASSES[1]({"a": "fifo"}).name == "MaxMinFairnessWaterFilling"


def test_the_flat_classes_name_the_new_ones():
    with pytest.raises(NotImplementedError, match="MaxMinFairnessWaterFillingHierarchicalPolicy"):
        wf.MaxMinFairnessWaterFillingPolicy({0: "fairness"})


@pytest.mark.parametrize("cls", CLASSES)
def test_small_case_by_hand(cls):
    """The entities split 5 workers 2 : 3; team a's D is 3, so it saturates at
    g = 2·(5/5) = 2 < 3: no; C* solves min(3, 2C) + min(3, 3C) = 5 → C = 1:
    g_a = 2, g_b = 3.  Team a, fairness over c = (1, 1): τ = 2/3, both jobs at
    2/3.  Team b, fifo, saturated: jobs 1, 2, 4 at 1."""
    c = small()
    eng = wfh_ref.TwinEngine()
    pol = cls(c["policies"], native=eng)
    out = pol.get_allocation(c["throughputs"], c["scale_factors"], c["priority_weights"], c["cluster_spec"],
                             entity_weights=c["entity_weights"], entity_to_job_mapping=c["entity_to_job_mapping"])
    got = [out[j]["v100"] for j in range(5)]
    assert got == pytest.approx([2 / 3, 1.0, 1.0, 2 / 3, 1.0], rel=1e-12)
    assert pol.last_entity_capacity == pytest.approx({"a": 2.0, "b": 3.0}, rel=1e-12)
    assert pol.last_level[0] == pytest.approx(1.0, rel=1e-12)
    (args, _), = eng.calls
    assert list(args[2]) == [0, 1, 1, 0, 1] and list(args[4]) == [0, 1] and args[5] == 5


def test_fifo_fills_in_ascending_job_id_whatever_the_mappings_order():
    c = small()
    c["cluster_spec"] = {"v100": 3}  # g_a = 1.2, g_b = 1.8: job 1 whole, job 2 at 0.8, job 4 waits
    out, pol = wc.policy_run(wfh_ref.TwinEngine(), c, "MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf")
    assert [out[j]["v100"] for j in (1, 2, 4)] == pytest.approx([1.0, 0.8, 0.0], abs=1e-12)


def test_errors():
    eng = wfh_ref.TwinEngine()
    c = small()
    call = lambda pol, **kw: pol.get_allocation(
        c["throughputs"], c["scale_factors"], c["priority_weights"], c["cluster_spec"],
        **{"entity_weights": c["entity_weights"], "entity_to_job_mapping": c["entity_to_job_mapping"], **kw})
    for cls in CLASSES:
        with pytest.raises(ValueError, match="Unknown priority reweighting policy"):
            cls({"a": "fairness", "b": "lifo"}, native=eng)
        with pytest.raises(ValueError):
            cls(None, native=eng)
        pol = cls(c["policies"], native=eng)
        with pytest.raises(ValueError, match="entity_to_job_mapping cannot be None"):
            call(pol, entity_to_job_mapping=None)
        with pytest.raises(ValueError, match="job 3 is in no entity"):
            call(pol, entity_to_job_mapping={"a": [0], "b": [4, 1, 2]})
        with pytest.raises(ValueError, match="job 1 is in two entities"):
            call(pol, entity_to_job_mapping={"a": [0, 3, 1], "b": [4, 1, 2]})
        with pytest.raises(ValueError, match="'c' has no priority reweighting policy"):
            call(pol, entity_to_job_mapping={"a": [0, 3], "b": [4, 1], "c": [2]})
        with pytest.raises(ValueError, match="weight"):
            call(pol, entity_weights={"a": 0.0, "b": 3.0})
        with pytest.raises(ValueError, match="weight"):
            call(pol, entity_weights={"a": 2.0})
    pol = CLASSES[0](c["policies"], native=eng)
    differ = {j: {"p100": 1.0, "v100": 1.0 + j} for j in range(5)}
    with pytest.raises(NotImplementedError):
        pol.get_allocation(differ, c["scale_factors"], c["priority_weights"], {"p100": 2, "v100": 3},
                           entity_weights=c["entity_weights"], entity_to_job_mapping=c["entity_to_job_mapping"])
    with pytest.raises(ValueError, match="job 2"):
        pol.get_allocation({**c["throughputs"], 2: {"v100": 0.0}}, c["scale_factors"], c["priority_weights"],
                           c["cluster_spec"], entity_weights=c["entity_weights"],
                           entity_to_job_mapping=c["entity_to_job_mapping"])
    with pytest.raises(ValueError, match="job 4"):
        pol.get_allocation(c["throughputs"], c["scale_factors"], {**c["priority_weights"], 4: 0.0},
                           c["cluster_spec"], entity_weights=c["entity_weights"],
                           entity_to_job_mapping=c["entity_to_job_mapping"])
    assert eng.calls == []


@pytest.mark.parametrize("cls", CLASSES)
def test_no_jobs_is_none(cls):
    pol = cls({"a": "fifo"}, native=wfh_ref.TwinEngine())
    assert pol.get_allocation({}, {}, {}, {"v100": 4}, entity_weights={"a": 1.0},
                              entity_to_job_mapping={"a": []}) is None


def test_several_identical_types_split_by_worker_count_and_effective_throughputs():
    c = small({j: {"p100": 3.0, "v100": 3.0} for j in range(5)})
    c["cluster_spec"] = {"p100": 1, "v100": 2}
    one = small()
    one["cluster_spec"] = {"v100": 3}
    for name in ("MaxMinFairnessWaterFillingHierarchicalPolicyWithPerf", "MaxMinFairnessWaterFillingHierarchicalPolicy"):
        out, _ = wc.policy_run(wfh_ref.TwinEngine(), c, name)
        ref, _ = wc.policy_run(wfh_ref.TwinEngine(), one, name)
        for j in range(5):
            assert out[j]["p100"] == ref[j]["v100"] * 1 / 3 and out[j]["v100"] == ref[j]["v100"] * 2 / 3
        (eff, ids), _ = wc.policy_run(wfh_ref.TwinEngine(), c, name, return_effective_throughputs=True)
        assert ids == [0, 1, 2, 3, 4]
        assert eff == pytest.approx([ref[j]["v100"] for j in ids], rel=1e-15, abs=1e-15)


def test_instance_of_the_references_hierarchical_test():
    """10 entities, 300 jobs, mixed modes, three worker types of 64: the
    unit-throughput class.  The shares are the twin's on the flattened
    instance, split by worker count, and the exact staged process's."""
    case = wc.policy_case()
    assert set(case["policies"].values()) == {"fairness", "fifo"}
    eng = wfh_ref.TwinEngine()
    out, pol = wc.policy_run(eng, case)
    (args, (x, g, level, used)), = eng.calls
    sf, c, ent, W, modes, G = args
    assert len(sf) == 300 and len(W) == 10 and G == 192 and int(np.sum(sf)) > G
    wc.check_properties(args, x, g, level, used)
    wc.check_against_fluid(args, x)
    for i in range(300):
        assert sum(out[i].values()) == pytest.approx(x[i], rel=1e-15, abs=1e-300)
        assert out[i]["k80"] == x[i] * 64 / 192
    assert math.fsum(pol.last_entity_capacity.values()) == pytest.approx(192, rel=1e-12)
    for e, name in enumerate(case["entity_to_job_mapping"]):
        assert sorted(np.flatnonzero(ent == e)) == sorted(case["entity_to_job_mapping"][name])
        assert modes[e] == (1 if case["policies"][name] == "fifo" else 0) and W[e] == case["entity_weights"][name]
