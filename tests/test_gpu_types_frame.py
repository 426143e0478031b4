"""The worker-type frame on the GPU (csrc/sw_types.h): what the four calls over
worker types that differ share on one handle.

  shared workspace   wf 40 × 16, centred mmf 5 × 3, ftf 513 × 2, mtd 1 × 1 on one
                     handle, then the same four in reverse: the workspace grows,
                     then a smaller call of another policy finds the larger one's
                     words in it; every result bit for bit the twin's
  error texts        for each of the eight entry points a table of bad calls with
                     the return code and the whole error text, calls with two
                     faults among them to fix which is reported; after every
                     refusal a good 5 × 3 call on the same handle equals its twin
"""
import functools

import numpy as np
import pytest

import ftftcases
import mmfccases
import mtdtcases
import wftcases

pytestmark = pytest.mark.gpu

CASES = {"mmf": mmfccases, "mtd": mtdtcases, "ftf": ftftcases, "wf": wftcases}
CALL = {"mmf": "mmf_allocate_types_centred", "mtd": "mtd_allocate_types", "ftf": "ftf_allocate_types",
        "wf": "wf_allocate_types"}
NOUT = {"mmf": 3, "mtd": 5, "ftf": 6, "wf": 6}  # the length of the solver's return tuple


@functools.lru_cache(maxsize=None)
def _case(policy, m, n):
    """The inputs and the twin's answer, computed once and left unchanged."""
    inst = tuple(CASES[policy].shaped(m, n))
    out = tuple(CASES[policy].twin_allocate(*inst))[:NOUT[policy]]
    for a in inst + out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inst, out


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if isinstance(b, np.ndarray):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
        elif isinstance(b, float):
            assert float(a).hex() == b.hex(), (a, b)
        else:
            assert a == b, (a, b)


def _good(solver, policy):
    inst, want = _case(policy, 5, 3)
    _same(getattr(solver, CALL[policy])(*inst), want)


def test_gpu_one_workspace_serves_the_four_policies(gpu_solver):
    order = [("wf", 40, 16), ("mmf", 5, 3), ("ftf", 513, 2), ("mtd", 1, 1)]
    for policy, m, n in order + order[::-1]:
        inst, want = _case(policy, m, n)
        got = getattr(gpu_solver, CALL[policy])(*inst)
        print(f"{policy} {m}x{n}: gpu {got[1:] if policy != 'wf' else got[2:]}")
        _same(got, want)
    for policy, m, n in order:  # and as batches of one, through the other four entry points
        inst, want = _case(policy, m, n)
        _same(getattr(gpu_solver, CALL[policy] + "_batch")([inst])[0], want)


# ---- the error texts, written out from the four calls' source ----
W2 = np.array([4, 2], dtype=np.int32)
NAN = float("nan")


def _inst(policy, m=3, W=W2, sf=None, nan_at=None, dead_at=None):
    """A small valid instance of the policy, or one with the named fault: a
    scale factor list, a NaN in the [m, n] column at job nan_at, a job dead_at
    without a coefficient on any type."""
    n = len(W)
    sf = np.ones(m, dtype=np.int32) if sf is None else np.asarray(sf, dtype=np.int32)
    c = 1.0 + np.arange(m * n, dtype=np.float64).reshape(m, n) / 8.0
    if nan_at is not None:
        c[nan_at, n - 1] = NAN
    if dead_at is not None:
        c[dead_at, :] = 0.0
    col = np.ones(m)
    return {"mmf": (W, sf, c), "wf": (W, sf, c), "mtd": (W, sf, c, 100.0 * col),
            "ftf": (W, sf, c, 100.0 * col, 10.0 * col, 50.0 * col)}[policy]


SF = "scale factors must be in [1,255]"
COEF = {"mmf": "coefficients must be finite and >= 0", "wf": "coefficients must be finite and >= 0",
        "mtd": "throughputs must be finite and >= 0", "ftf": "throughputs must be finite and >= 0"}
DEAD = {"mtd": "a job with steps left has no throughput on a type with workers",
        "ftf": "a job with steps left has no throughput on a type with workers",
        "wf": "a job has no positive coefficient on a type with workers"}
NAMES_JOB = {"mmf": False, "mtd": False, "ftf": True, "wf": True}  # the sf and value texts name the job


def _at(policy, job, inst, always=False):
    return f" (job {job} of instance {inst})" if always or NAMES_JOB[policy] else ""


def _refused(solver, policy, fn, args, text, kw=None):
    import sw_native as sn

    who = "sw_" + fn
    with pytest.raises(sn.NativeError) as e:
        getattr(solver, fn)(*args, **(kw or {}))
    assert e.value.code == sn.SW_ERR_INVALID
    assert solver.error() == f"{who}: {text}", solver.error()
    assert str(e.value) == f"{who} failed ({sn.SW_ERR_INVALID}): {who}: {text}"
    _good(solver, policy)


@pytest.mark.parametrize("policy", list(CASES))
def test_gpu_single_call_error_texts(gpu_solver, policy):
    fn = CALL[policy]
    bad = functools.partial(_refused, gpu_solver, policy, fn)
    bad(_inst(policy, sf=[1, 0, 1]), SF + _at(policy, 1, 0))
    bad(_inst(policy, sf=[256, 1, 1]), SF + _at(policy, 0, 0))
    bad(_inst(policy, nan_at=2), COEF[policy] + _at(policy, 2, 0))
    # two faults: the worker counts come before any value of a job
    bad(_inst(policy, W=np.array([4, -1], dtype=np.int32), nan_at=0), "worker counts must be >= 0")
    bad(_inst(policy, W=np.array([4, -1], dtype=np.int32), sf=[0, 1, 1]), "worker counts must be >= 0")
    # two faults in one job: FinishTimeFairness reads the throughputs first, the others the scale factor
    both = _inst(policy, sf=[1, 0, 1], nan_at=1)
    bad(both, (COEF[policy] if policy == "ftf" else SF) + _at(policy, 1, 0))
    # two faults in two jobs: the earlier job's
    bad(_inst(policy, sf=[1, 1, 0], nan_at=0), COEF[policy] + _at(policy, 0, 0))
    if policy in DEAD:
        bad(_inst(policy, dead_at=1), DEAD[policy] + _at(policy, 1, 0, always=True))
    bad(_inst(policy, W=np.full(17, 8, dtype=np.int32)), "bad sizes or null pointers")
    bad(_inst(policy, m=16385, W=np.array([4], dtype=np.int32)), "more than 16384 jobs in an instance")


@pytest.mark.parametrize("policy", list(CASES))
def test_gpu_batch_call_error_texts(gpu_solver, policy):
    fn = CALL[policy] + "_batch"
    bad = functools.partial(_refused, gpu_solver, policy, fn)
    ok = _inst(policy)
    # a bad offset and a bad scale factor: the offsets come first
    sf0 = _inst(policy, sf=[0, 1, 1])
    bad(([sf0, ok],), "offsets must start at 0", kw={"offsets": [1, 3, 6]})
    bad(([sf0, ok],), "offsets must not decrease", kw={"offsets": [0, 4, 3]})
    bad(([sf0, ok],), "offsets must not decrease", kw={"offsets": [0, -1, 6]})
    # a negative worker count in instance 1 and a NaN coefficient in instance 0
    bad(([_inst(policy, nan_at=0), _inst(policy, W=np.array([4, -1], dtype=np.int32))],),
        "worker counts must be >= 0")
    # an offset fault of instance 1 after a worker fault of instance 0: instance by instance
    bad(([_inst(policy, W=np.array([-4, 1], dtype=np.int32)), ok],), "worker counts must be >= 0",
        kw={"offsets": [0, 3, 2]})
    # faults in job 0 of instance 1 and in job 2 of instance 0: the scans go instance by instance
    bad(([_inst(policy, sf=[1, 1, 0]), _inst(policy, nan_at=0)],), SF + _at(policy, 2, 0))
    bad(([_inst(policy, nan_at=2), _inst(policy, sf=[0, 1, 1])],), COEF[policy] + _at(policy, 2, 0))
    bad(([ok, _inst(policy, sf=[300, 1, 1])],), SF + _at(policy, 0, 1))
    if policy in DEAD:
        bad(([ok, _inst(policy, m=0), _inst(policy, dead_at=2)],), DEAD[policy] + _at(policy, 2, 2, always=True))
