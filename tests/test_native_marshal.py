"""What sw_native.py hands to C and what it makes of the answer, on the CPU,
against tests/golden/native_marshal.json (written by
tests/golden/make_native_marshal.py from ``record()`` below, at the commit
before the binding was moved onto its signature and policy tables).

Signatures: restype and argtypes of every name in ``EXPORTED_SYMBOLS`` after
``load()``.

Calls: ``Solver(lib=FakeLib())``.  Every ``sw_*`` function of the fake records
its name, its scalars and, for each pointer, the ctypes type, whether it is
null, the size of the numpy array behind it and the bytes C would read (as hex,
a run of one byte as "xx*n"), then
fills each output with ``position_in_call + index * 2**-10`` (integer arrays
with 1024 times that, modulo the type's range), so that the slicing per
instance shows in what the method returns.  How long each pointer is comes from
``SHAPES``, written from the shapes include/shockwave_amd.h documents; a buffer
shorter than its documented shape fails the test before anything is read.  The
method's return value is recorded with types and shapes, every float as
``float.hex``, and each returned array with whether it is memory C wrote to (a
single call's outputs) or a copy (a batch's).  Every recorded argument is also
offered to ``from_param`` of the real library's declared argtype.

An ``offsets=`` override keeps the last entry of the offsets it replaces: the
shapes follow the offsets C is given, and the arrays are as long as the
instances make them.
"""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import sw_native as sn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_marshal.json")
LAST_ERROR = b"the fake library's last error"


def _types_shapes(stem, cols, extra, width):
    """The single and the batch form of a worker-type policy: workers, scale
    factors, the [m, n] column, the [m] columns, allocation, extra output, result."""
    per_job = "".join(f" {c}<[m]" for c in cols)
    per_job_b = "".join(f" {c}<[off[-1]]" for c in cols)
    one = {"": "", "levels": " levels>[m]", "prices": " prices>[n]"}[extra]
    many = {"": "", "levels": " levels>[off[-1]]", "prices": " prices>[count*n]"}[extra]
    return {f"sw_{stem}": f"h m n workers<[n] sf<[m] c<[m*n]{per_job} x>[m*n]{one} result>[{width}]",
            f"sw_{stem}_batch": f"h count n off<[count+1] workers<[count*n] sf<[off[-1]] c<[off[-1]*n]{per_job_b} "
                                f"x>[off[-1]*n]{many} results>[count*{width}]"}


def _alloc_shapes(stem, cols, width):
    """The single and the batch form of a per-job policy."""
    return {f"sw_{stem}_allocate": "h m g" + "".join(f" {c}<[m]" for c in cols) + f" x>[m] level>[{width}]",
            f"sw_{stem}_allocate_batch": "h count off<[count+1] g<[count]" +
                                         "".join(f" {c}<[off[-1]]" for c in cols) +
                                         f" x>[off[-1]] levels>[count*{width}]"}


# name → the arguments in order: a scalar's name, name<[length] for memory C
# reads, name>[length] for memory C writes; lengths in the scalars and the
# arrays already named.  P is an sw_problem, R the sw_result of the problem at
# the same place (of the last upload where the call has no problems).
SHAPES = {
    "sw_destroy": "h",
    "sw_plan_solve": "h prob<P res>R",
    "sw_plan_solve_batch": "h count probs<P res>R",
    "sw_batch_upload": "h count probs<P",
    "sw_batch_run": "h",
    "sw_batch_download": "h res>R",
    "sw_batch_keep_masks": "h keep",
    "sw_stream": "h",
    "sw_set_timing": "h enable",
    "sw_kernel_times": "h ms_p2x>[1] ms_plan>[1] runs>[1]",
    "sw_dist_plan_solve": "h prob<P job_offset total_jobs res>R",
    "sw_dist_enable_peer": "h max_total_jobs",
    "sw_mmf_allocate": "h m g sf<[m] c<[m] x>[m] level>[2]",
    **_types_shapes("mmf_allocate_types", (), "", 2),
    **_types_shapes("mmf_allocate_types_centred", (), "", 2),
    **_types_shapes("mtd_allocate_types", ("steps",), "", 4),
    **_types_shapes("ftf_allocate_types", ("steps", "elapsed", "expected"), "", 5),
    **_types_shapes("wf_allocate_types", (), "levels", 4),
    **_types_shapes("mst_allocate_types", (), "prices", 4),
    **_alloc_shapes("ftf", ("sf", "full_time", "elapsed", "isolated_time"), 2),
    **_alloc_shapes("wf", ("sf", "c"), 2),
    **_alloc_shapes("mtd", ("sf", "full_time"), 2),
    **_alloc_shapes("mst", ("sf", "weights", "floors"), 4),
    "sw_wfh_allocate": "h m ne g sf<[m] c<[m] ent<[m] w<[ne] modes<[ne] x>[m] cap>[ne] level>[2]",
    "sw_wfh_allocate_batch": "h count off<[count+1] eoff<[count+1] g<[count] sf<[off[-1]] c<[off[-1]] ent<[off[-1]] "
                             "w<[eoff[-1]] modes<[eoff[-1]] x>[off[-1]] cap>[eoff[-1]] levels>[count*2]",
    "sw_allox_assign": "h m nt free<[nt] p<[m*nt] d<[m] jw>[m] jp>[m] wf>[free.clip(0).sum()] cost>[1]",
    "sw_allox_assign_batch": "h count joff<[count+1] nt<[count] free<[count*8] p<[np.dot(np.diff(joff),nt)] "
                             "d<[joff[-1]] jw>[joff[-1]] jp>[joff[-1]] wf>[woff[-1]] woff<[count+1] costs>[count]",
}
del SHAPES["sw_mmf_allocate_types_batch"]  # the simplex form has a single call only


def _hex(b):
    """The bytes as hex; n equal bytes as "xx*n"."""
    return f"{b[0]:02x}*{len(b)}" if len(b) > 8 and len(set(b)) == 1 else b.hex()


def _fill(position, length, dtype, shift=0):
    v = position + (np.arange(length) + shift) * 2.0 ** -10
    return v if np.dtype(dtype).kind == "f" else (v * 1024).astype(np.int64).astype(dtype)


class FakeLib:
    """The recorder (see the module's docstring); rc is what every call returns."""

    def __init__(self, real, rc=0):
        self._real, self._rc = real, rc
        self.calls, self.written, self._uploaded = [], [], []

    def sw_create(self, cfg):
        return 1

    def sw_create_error(self):
        return None

    def sw_last_error(self, h):
        return LAST_ERROR

    def __getattr__(self, name):
        if name not in SHAPES:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _memory(self, arg, position, length, out, argtype):
        """[type, null, size of the array behind it, the bytes]; fills an output."""
        if arg is None:
            return [argtype.__name__, True, None, ""]
        scalar = getattr(arg, "_obj", None)  # byref(c_double()) and the like
        if scalar is not None:
            assert length == 1
            before = _hex(bytes(scalar))
            if out:
                scalar.value = _fill(position, 1, type(scalar))[0].item()
            return ["byref(" + type(scalar).__name__ + ")", False, None, before]
        behind = getattr(arg, "_arr", None)
        assert behind is None or behind.size >= length, (behind.size, length)
        if behind is not None:
            self.written.append(behind)
        if not arg or not length:
            return [type(arg).__name__, not arg, None if behind is None else behind.size, ""]
        mem = np.ctypeslib.as_array(arg, (length,))
        before = _hex(mem.tobytes())
        if out:
            mem[:] = _fill(position, length, mem.dtype)
        return [type(arg).__name__, False, None if behind is None else behind.size, before]

    def _problem(self, p):
        nj, nb = p.num_jobs, p.num_bases
        return {"scalars": [nj, p.future_rounds, p.num_gpus, nb, p.round_duration.hex(), p.regularizer.hex()],
                **{f: self._memory(getattr(p, f), 0, nb if "bases" in f else nj, False, None)
                   for f in ("bases", "log_bases", "nworkers", "epoch_duration", "completed_epochs", "total_epochs",
                             "remaining_runtime", "priority")}}

    def _result(self, r, i, position, dims):
        nj, rounds = dims
        rec = {f: self._memory(getattr(r, f), position, n, True, t)
               for f, n, t in (("plan", nj * rounds, C.POINTER(C.c_uint8)),
                               ("planned_rounds", nj, C.POINTER(C.c_int32)),
                               ("plan_masks", nj, C.POINTER(C.c_uint64)))}
        for k, f in enumerate(("objective", "utility", "makespan", "p2_objective", "bound")):
            setattr(r, f, position + i * 2.0 ** -10 + (k + 1) * 2.0 ** -4)
        r.iters, r.status = position * 1024 + i, i
        return rec

    def _call(self, name, *args):
        real = getattr(self._real, name)
        spec = [re.fullmatch(r"(\w+)(?:([<>])(P|R|\[(.*)\]))?", t).groups() for t in SHAPES[name].split()]
        assert len(spec) == len(args), (name, len(args))
        for t, a in zip(real.argtypes or (), args):
            t.from_param(a)  # raises where the real library would refuse the argument
        env, rec, count = {"np": np}, [None] * len(args), None
        # what C reads first (lengths may name an array that comes later), then what it writes
        for out in (False, True):
            for k, ((arg_name, way, kind, length), a) in enumerate(zip(spec, args)):
                if way is None:
                    if not out:
                        rec[k] = env[arg_name] = a.value if isinstance(a, C.c_void_p) else a
                        assert isinstance(rec[k], int), (name, arg_name)
                        count = a if arg_name == "count" else count
                elif (way == ">") != out:
                    continue
                elif kind == "P":
                    probs = [a._obj] if count is None else list(a)[:count]
                    rec[k] = [self._problem(p) for p in probs]
                    dims = [(p.num_jobs, p.future_rounds) for p in probs]
                    if name == "sw_batch_upload":
                        self._uploaded = dims
                elif kind == "R":
                    dims = self._uploaded if name == "sw_batch_download" else dims
                    ress = [a._obj] if hasattr(a, "_obj") else list(a)[:len(dims)]
                    rec[k] = [self._result(r, i, k, d) for i, (r, d) in enumerate(zip(ress, dims))]
                else:
                    n = int(eval(length, dict(env)))
                    rec[k] = self._memory(a, k, n, out, real.argtypes[k])
                    if not out and a is not None:
                        env[arg_name] = np.ctypeslib.as_array(a, (n,)) if n else np.zeros(0, dtype=np.int64)
        self.calls.append([name] + rec)
        return self._rc


def _enc(v, written):
    """The value as JSON with its types: floats as float.hex, arrays with dtype,
    shape, bytes and whether C wrote into their memory."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, np.ndarray):
        passed = any(v is w or v.base is w for w in written)
        return {"array": v.dtype.str, "shape": list(v.shape), "bytes": _hex(v.tobytes()), "passed_to_c": passed}
    if isinstance(v, np.generic):
        return {type(v).__name__: _enc(v.item(), written)}
    if isinstance(v, dict):
        return {"dict": {k: _enc(x, written) for k, x in v.items()}}
    if isinstance(v, (list, tuple)):
        return {type(v).__name__: [_enc(x, written) for x in v]}
    raise TypeError(type(v))


# ---- the inputs: 3 jobs × 2 types, 2 entities; batches of lengths (2, 0, 3) ----
def _types_inst(m, k, cols, n=2):
    """(workers, scale factors, the [m, n] column, cols [m] columns) in dtypes
    and layouts the binding has to convert."""
    c = np.asfortranarray(((np.arange(m * n) + 1 + 10 * k) / 8).reshape(m, n).astype(np.float32))
    return ([2 + k, 3, 1][:n], np.arange(1, m + 1, dtype=np.int64), c) + \
        tuple([float(j + 2 * i + k) for j in range(m)] for i in range(cols))


def _alloc_inst(m, k, dtypes):
    return tuple(np.arange(1, m + 1, dtype=np.int64) if t == "i" else
                 (np.arange(m, dtype=np.float32) + i + k) / 4 for i, t in enumerate(dtypes))


def _wfh_inst(m, ne, k):
    return (list(range(1, m + 1)), [0.5 * (j + 1) + k for j in range(m)], [j % max(ne, 1) for j in range(m)],
            [1.0 + e + k for e in range(ne)], np.arange(ne, dtype=np.int64) % 2, 4 + k)


def _allox_inst(m, free, k):
    nt = len(free)
    return free, np.asfortranarray(((np.arange(m * nt) + k) / 2).reshape(m, nt)), [float(j + k) for j in range(m)]


def _problem(n, seed):
    return sn.ProblemArrays(np.arange(1, n + 1, dtype=np.int64), [10.0 + seed + j for j in range(n)],
                            [j for j in range(n)], [5 + j for j in range(n)], [100.0 * (j + 1) for j in range(n)],
                            np.ones(n, dtype=np.float32), future_rounds=4, num_gpus=8, round_duration=120.0,
                            regularizer=1e-3)


def _arrays_fields(a):
    return {f: getattr(a, f) for f in ("w", "d", "F", "E", "R", "p", "T", "G", "delta", "k", "bases", "ell", "N",
                                       "plan", "planned")}


LENGTHS = (2, 0, 3)
OVERRIDE = [0, 1, 3, 5]  # not the built [0, 2, 2, 5]: C gets these, the slices stay the built ones
TYPES = {"mmf_allocate_types_centred": 0, "mtd_allocate_types": 1, "ftf_allocate_types": 3, "wf_allocate_types": 0,
         "mst_allocate_types": 0}
ALLOC = {"ftf_allocate": "ifff", "wf_allocate": "if", "mtd_allocate": "if", "mst_allocate": "iff"}


def _scenarios():
    """name → what to do with a solver."""
    sc = {}

    def batch(make):
        return [make(m, k) for k, m in enumerate(LENGTHS)]

    sc["mmf_allocate"] = lambda s: s.mmf_allocate(np.arange(1, 4, dtype=np.int64), [0.5, 1.0, 1.5], 4.0)
    sc["mmf_allocate/length"] = lambda s: s.mmf_allocate([1, 2, 3], [0.5, 1.0], 4)
    sc["mmf_allocate_types"] = lambda s: s.mmf_allocate_types(*_types_inst(3, 0, 0))
    sc["mmf_allocate_types/shape"] = lambda s: s.mmf_allocate_types([2, 3], [1, 2, 3], np.ones((2, 3)))
    for name, cols in TYPES.items():
        one = functools.partial(_types_inst, cols=cols)
        sc[name] = lambda s, name=name, one=one: getattr(s, name)(*one(3, 0))
        sc[name + "/flat_column"] = lambda s, name=name, one=one: getattr(s, name)(
            *(np.ravel(v) if i == 2 else v for i, v in enumerate(one(3, 0))))
        sc[name + "/wrong_jobs"] = lambda s, name=name, one=one: getattr(s, name)(
            *(v[:2] if i == 1 else v for i, v in enumerate(one(3, 0))))
        for c in range(cols):
            sc[f"{name}/short_column_{c}"] = lambda s, name=name, one=one, c=c: getattr(s, name)(
                *(v[:2] if i == 3 + c else v for i, v in enumerate(one(3, 0))))
        sc[name + "_batch"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(batch(one))
        sc[name + "_batch/empty"] = lambda s, name=name: getattr(s, name + "_batch")([])
        sc[name + "_batch/offsets"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(
            batch(one), offsets=OVERRIDE)
        sc[name + "_batch/types_differ"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(
            [one(2, 0), one(3, 1, n=3)])
        # the shape error of the second instance is found before the differing number of types
        sc[name + "_batch/shape_before_types"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(
            [one(2, 0), one(3, 1, n=3)[:2] + (np.ones((2, 2)),) + one(3, 1, n=3)[3:]])
        sc[name + "_batch/native_error"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(batch(one))
    for name, dtypes in ALLOC.items():
        one = functools.partial(_alloc_inst, dtypes=dtypes)
        sc[name] = lambda s, name=name, one=one: getattr(s, name)(*one(3, 0), 4)
        sc[name + "/length"] = lambda s, name=name, one=one: getattr(s, name)(*one(3, 0)[:-1], one(2, 0)[-1], 4)
        sc[name + "_batch"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(
            [one(m, k) + (4.0 + k,) for k, m in enumerate(LENGTHS)])
        sc[name + "_batch/empty"] = lambda s, name=name: getattr(s, name + "_batch")([])
        sc[name + "_batch/offsets"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(
            [one(m, k) + (4 + k,) for k, m in enumerate(LENGTHS)], offsets=np.array(OVERRIDE, dtype=np.int32))
        sc[name + "_batch/length"] = lambda s, name=name, one=one: getattr(s, name + "_batch")(
            [one(2, 0) + (4,), one(3, 0)[:-1] + (one(2, 0)[-1], 4)])
    sc["mst_allocate/no_floors"] = lambda s: s.mst_allocate([1, 2, 4], [1.0, 2.0, 3.0], None, 4)
    sc["mst_allocate_batch/no_floors"] = lambda s: s.mst_allocate_batch(
        [_alloc_inst(m, k, "if") + (None, 4 + k) for k, m in enumerate(LENGTHS)])
    sc["mst_allocate_batch/no_floors_in_one"] = lambda s: s.mst_allocate_batch(
        [_alloc_inst(m, k, "iff")[:2] + (None if k == 2 else _alloc_inst(m, k, "iff")[2], 4 + k)
         for k, m in enumerate(LENGTHS)])
    sc["mst_allocate/native_error"] = lambda s: s.mst_allocate([1, 2, 4], [1.0, 2.0, 3.0], None, 4)
    sc["wfh_allocate"] = lambda s: s.wfh_allocate(*_wfh_inst(3, 2, 0))
    sc["wfh_allocate/job_lengths"] = lambda s: s.wfh_allocate([1, 2, 3], [1.0, 2.0, 3.0], [0, 1], [1.0, 2.0], [0, 1], 4)
    sc["wfh_allocate/entity_lengths"] = lambda s: s.wfh_allocate([1, 2, 3], [1.0, 2.0, 3.0], [0, 1, 0], [1.0, 2.0],
                                                                 [0], 4)
    sc["wfh_allocate/both_lengths"] = lambda s: s.wfh_allocate([1, 2, 3], [1.0, 2.0], [0, 1, 0], [1.0, 2.0], [0], 4)
    wfh = [_wfh_inst(m, ne, k) for k, (m, ne) in enumerate(zip(LENGTHS, (2, 0, 2)))]
    sc["wfh_allocate_batch"] = lambda s: s.wfh_allocate_batch(wfh)
    sc["wfh_allocate_batch/empty"] = lambda s: s.wfh_allocate_batch([])
    sc["wfh_allocate_batch/offsets"] = lambda s: s.wfh_allocate_batch(wfh, job_offsets=OVERRIDE,
                                                                      entity_offsets=[0, 1, 3, 4])
    sc["wfh_allocate_batch/job_offsets"] = lambda s: s.wfh_allocate_batch(wfh, job_offsets=OVERRIDE)
    sc["wfh_allocate_batch/length"] = lambda s: s.wfh_allocate_batch([wfh[0], wfh[2][:3] + ([1.0], [0, 1], 4)])
    sc["wfh_allocate_batch/native_error"] = lambda s: s.wfh_allocate_batch(wfh)
    sc["allox_assign"] = lambda s: s.allox_assign(*_allox_inst(3, [2, 1], 0))
    sc["allox_assign/zero_and_negative_free"] = lambda s: s.allox_assign(*_allox_inst(3, [0, -2], 0))
    sc["allox_assign/free_as_scalar_rows"] = lambda s: s.allox_assign(np.array([[2], [1]]), np.arange(6.0),
                                                                      np.ones((3, 1)))
    sc["allox_assign/shape"] = lambda s: s.allox_assign([2, 1], np.ones((3, 3)), [0.0, 1.0, 2.0])
    allox = [_allox_inst(m, free, k) for k, (m, free) in enumerate(zip(LENGTHS, ([2, 1], [0, -2, 3], [1])))]
    sc["allox_assign_batch"] = lambda s: s.allox_assign_batch(allox)
    sc["allox_assign_batch/empty"] = lambda s: s.allox_assign_batch([])
    sc["allox_assign_batch/no_free_workers"] = lambda s: s.allox_assign_batch([_allox_inst(2, [0, -1], 0)])
    sc["allox_assign_batch/nine_types"] = lambda s: s.allox_assign_batch([allox[0], _allox_inst(2, [1] * 9, 0)])
    # the shape error of the second instance is found before the first one's nine types
    sc["allox_assign_batch/shape_before_types"] = lambda s: s.allox_assign_batch(
        [_allox_inst(2, [1] * 9, 0), ([2, 1], np.ones((3, 3)), [0.0, 1.0, 2.0])])
    sc["allox_assign_batch/native_error"] = lambda s: s.allox_assign_batch(allox)
    sc["solve"] = lambda s: s.solve(_problem(3, 0))
    sc["solve/native_error"] = lambda s: s.solve(_problem(3, 0))
    sc["solve_batch"] = lambda s: s.solve_batch([_problem(3, 0), _problem(2, 1)])
    sc["solve_batch/masks_no_plan"] = lambda s: s.solve_batch([_problem(3, 0), _problem(2, 1)], masks=True,
                                                              plan=False)

    def device_batch(s):
        s.upload([_problem(3, 0), _problem(2, 1), _problem(0, 2)])
        s.run()
        s.keep_masks(True)
        return s.download(masks=True), s.download()

    sc["upload_run_download"] = device_batch
    sc["slice"] = lambda s: _arrays_fields(_problem(3, 0).slice(1, 3))
    sc["slice/solve"] = lambda s: s.solve(_problem(3, 0).slice(1, 3))
    sc["problem/lengths"] = lambda s: sn.ProblemArrays([1, 2], [1.0, 2.0], [0, 0], [5, 5], [10.0], [1.0, 1.0], 4, 8,
                                                       120.0, 1e-3)
    sc["dist_solve"] = lambda s: s.dist_solve(_problem(3, 0).slice(1, 3), 1, 3)
    sc["small_calls"] = lambda s: (s.stream(), s.set_timing(True), s.kernel_times(), s.dist_enable_peer(7),
                                   s.error())
    return sc


SCENARIOS = _scenarios()


def record_signatures():
    lib = sn.load()
    out = {}
    for name in sn.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        out[name] = ["None" if fn.restype is None else fn.restype.__name__, [t.__name__ for t in fn.argtypes or ()]]
    return out


def record_scenario(name):
    fake = FakeLib(sn.load(), rc=-1 if name.endswith("/native_error") else 0)
    solver = sn.Solver(lib=fake)
    try:
        r = {"returns": _enc(SCENARIOS[name](solver), fake.written)}
    except (ValueError, sn.NativeError) as exc:  # the type, the text and the code are what is compared
        r = {"raises": [type(exc).__name__, str(exc), getattr(exc, "code", None)]}
    r["calls"] = fake.calls[:]
    solver.close()
    assert fake.calls[len(r["calls"]):] == [["sw_destroy", 1]]
    return json.loads(json.dumps(r))  # as the fixture holds it: tuples are lists


def record():
    return {"signatures": record_signatures(), "scenarios": {name: record_scenario(name) for name in SCENARIOS}}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_signatures_match_the_recording():
    got, want = record_signatures(), _golden()["signatures"]
    assert sorted(got) == sorted(want) == sorted(sn.EXPORTED_SYMBOLS)
    for name in want:
        assert got[name] == want[name], name


def test_every_scenario_is_recorded():
    assert sorted(SCENARIOS) == sorted(_golden()["scenarios"])


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_call_matches_the_recording(name):
    assert record_scenario(name) == _golden()["scenarios"][name]


def test_the_recording_covers_the_binding():
    """Every public allocation method of Solver, single and batch, reached C in
    some scenario; every ValueError text of the binding and a NativeError with
    its code were recorded."""
    scenarios = _golden()["scenarios"]
    called = {c[0] for r in scenarios.values() for c in r["calls"]}
    public = {n for n in vars(sn.Solver) if re.fullmatch(r"[a-z]+_(allocate|assign)\w*", n)}
    assert public and {"sw_" + n for n in public} <= called
    assert called >= {"sw_plan_solve", "sw_plan_solve_batch", "sw_batch_upload", "sw_batch_download"}
    raised = {tuple(r["raises"][:2]) for r in scenarios.values() if "raises" in r}
    texts = {t for k, t in raised if k == "ValueError"}
    assert {"every instance must have the same number of worker types", "at most 8 worker types",
            "coefficients must be [num_jobs][num_types]", "weights must be [num_jobs][num_types]",
            "throughputs must be [num_jobs][num_types], steps [num_jobs]",
            "throughputs must be [num_jobs][num_types], steps, elapsed and expected [num_jobs]",
            "scale_factors and coefficients must have the same length",
            "scale_factors, full_time, elapsed and isolated_time must have the same length",
            "scale_factors and full_time must have the same length",
            "scale_factors, weights and floors must have the same length",
            "scale_factors, coefficients and entity_of_job must have the same length",
            "entity_weights and entity_modes must have the same length",
            "proc_time must be [len(delay)][len(free_workers)]",
            "per-job arrays must have the same length"} == texts
    assert all(r["calls"] == [] for r in scenarios.values() if r.get("raises", [""])[0] == "ValueError")
    native = [r["raises"] for r in scenarios.values() if r.get("raises", [""])[0] == "NativeError"]
    assert len(native) >= 8 and all(code == -1 and LAST_ERROR.decode() in text for _, text, code in native)
