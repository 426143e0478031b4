"""Instances that walk the sharded GPU engine's size-selected launch forms
(test data and a restatement of the dispatch, no product logic).

csrc/sw_shard.hip picks the kernels of a placement by its size: pack_any and
pack_share_any by the entries per workgroup and, inside the kernels, by the
active entries A (jobs with rounds to place).  The CPU shard engine
(oracle/shard_twin.c) has one loop for all of them, and records per solve the
sizes that decide (shard_twin_record).  `launch_forms` maps such a record to
the names of the forms the GPU engine takes on the same instance; `CASES`
is chosen (on the CPU, tests/test_shard_ladder.py asserts it) so that the
union of the names is `ALL_FORMS`.
"""
import ctypes

import numpy as np

import sw_native as sn
import sw_synth as ss

BASES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
LANES = 512      # SW_DET_LANES
BLOCK = 512      # SW_BLOCK, threads of a round-loop workgroup
WAVE_A = 512     # wave_pack_max(): active entries the one-wave loop places
CHUNK = 256      # kSortChunk
MERGE_G = 64     # kMergeG: chunks one pass of the merge's lanes covers


# ---- the generators ---------------------------------------------------------

def short_problem(seed, N, G=511, T=64, k=1.0, widths=(1,), done=0, idle=0, lam=5.0, delta=120.0):
    """Jobs that one round finishes (E − F in 1..3 epochs of 5..200 s at
    Δ = 120 s): the level search gives every job a round, so nearly all N jobs
    are active in the placement — where the trace-shaped generators put a few
    hundred of 12,000 jobs in the plan, because G·T binds first.  `done`: that
    many jobs (spread evenly) are finished (F = E; their keys are zero, they
    take rounds only where capacity is left over).  `idle`: that many jobs
    (spread evenly) are wider than the cluster, which never take an entry:
    A ≤ N − idle exactly."""
    rng = np.random.default_rng(77_000_003 + seed)
    w = rng.choice(np.asarray(widths, dtype=np.int32), size=N).astype(np.int32)
    left = rng.integers(1, 4, size=N).astype(np.int32)
    F = rng.integers(0, 50, size=N).astype(np.int32)
    E = (F + left).astype(np.int32)
    d = np.round(rng.uniform(5.0, 200.0, size=N))
    if done:
        idx = np.linspace(0, N - 1, done).astype(np.int64)
        F[idx] = E[idx]
        left[idx] = 0
    R = left * d * rng.uniform(0.7, 1.3, size=N)
    p = np.exp(rng.normal(np.log(1.5), 0.45, size=N)) ** lam
    if idle:
        w[np.linspace(0, N - 1, idle).astype(np.int64)] = G + 1
    return sn.ProblemArrays(w, d, F, E, R, p, T, G, delta, k, BASES)


def build(case):
    """A case's instance: case = (name, kind, args)."""
    _, kind, args = case
    if kind == "short":
        return short_problem(**args)
    if kind == "synth":
        a = dict(args)
        return ss.synth_problem(a.pop("seed"), a.pop("N"), a.pop("G"), a.pop("T"), 120.0, a.pop("k"),
                                a.pop("lam", 5.0), **a)
    if kind == "fuzz":
        from fuzzcases import fuzz_problem
        return fuzz_problem(args["seed"], max_n=args["N"], min_n=args["N"],
                            trace_widths=args.get("trace_widths", False))
    raise ValueError(kind)


# ---- the CPU engine's record ------------------------------------------------

RR_KEYS = ("runs", "cap_max", "words2", "cap512", "refused_capmax", "refused_words", "refused_budget",
           "levels_max")


def read_record(lib):
    """shard_twin_record of the last solve whose rank 0 ran in this process."""
    fn = lib.shard_twin_record
    fn.restype = ctypes.c_int64
    fn.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]
    n = fn(None, 0)
    buf = (ctypes.c_int64 * n)()
    fn(buf, n)
    v = list(buf)
    rec = dict(dropped=v[1], reround_calls=v[2], rr=dict(zip(RR_KEYS, v[3:11])), p2x_runs=v[11],
               p2x_jobs=v[12], shares=[], packs=[], share_class_packs=[])
    for e in range(16, n, 4):
        kind, a, b, c = v[e:e + 4]
        if kind == 0:
            rec["shares"].append(dict(V=a, nsub=b, exist=c, A=[]))
        elif kind == 3:
            rec["shares"][-1]["A"].append((b, c))  # (jobs, active) of rank 0's share a
        elif kind == 1:
            rec["packs"].append(dict(mode=a, M=b, A=c))
        elif kind == 2:
            rec["share_class_packs"].append(dict(width=a, jobs=b, A=c))
    return rec


# ---- the dispatch, restated -------------------------------------------------

def share_count(N, G, world):
    """sw_share_count (csrc/sw_shard_ctl.h)."""
    return 8 if world < 8 and 4096 <= N <= 65536 and G >= 512 else world


def sizes(N, world, G):
    """prepare()'s sizes: q jobs per lane, M gathered entries, nsub shares on
    a rank of Mg entries each."""
    q = max(1, -(-N // LANES))
    V = share_count(N, G, world)
    nsub = V // world
    P = (LANES // world) * q
    Mg = P if nsub == 1 else -(-((LANES // V) * q) // CHUNK) * CHUNK
    return dict(q=q, V=V, nsub=nsub, P=P, M=P * world, Mg=Mg)


def _body(A, top):
    """k_pack_rounds_sel's body for A active entries (top: the widest)."""
    return 2 if A <= 2 * BLOCK else 4 if A <= 4 * BLOCK else 8 if A <= 8 * BLOCK else top


def share_form(Mg, nsub, A):
    """pack_share_any → pack_any(shares): the form that places a share of Mg
    entries, A of them active."""
    if Mg <= 8 * BLOCK:  # k_pack_rounds_share, one launch
        return "S1/wave" if A <= WAVE_A else f"S1/body{_body(A, 8)}"
    if Mg > (20 if nsub > 1 else 64) * BLOCK:
        return "S5/refused"
    if Mg <= 20 * BLOCK:  # k_share_caps, k_pack_rounds_wave, k_pack_rounds_sel<512,20>
        return "S2/wave" if A <= WAVE_A else f"S2/body{_body(A, 20)}"
    f, e = ("S3", 32) if Mg <= 32 * BLOCK else ("S4", 64)
    if A <= WAVE_A:
        return f"{f}/wave"
    return f"{f}/sel{_body(A, 8)}" if A <= 8 * BLOCK else f"{f}/rounds{e}"


def gathered_form(M, A):
    """pack_any without shares: M entries, A active."""
    if M <= WAVE_A:
        return "G1/wave"
    if M <= 4 * WAVE_A:
        return "G2/wave" if A <= WAVE_A else f"G2/body{_body(A, 8)}"
    if M <= 8 * BLOCK:
        return f"G3/body{_body(A, 8)}"
    if M <= 20 * BLOCK:
        return f"G4/body{_body(A, 20)}"
    if M > 64 * BLOCK:
        return "G7/refused"
    f, e = ("G5", 32) if M <= 32 * BLOCK else ("G6", 64)
    return f"{f}/sel{_body(A, 8)}" if A <= 8 * BLOCK else f"{f}/rounds{e}"


def launch_forms(N, world, G, record):
    """The names of the launch forms the GPU engine takes, at rank 0 of
    `world`, on an instance whose CPU solve left `record`."""
    z = sizes(N, world, G)
    out = set()
    for sh in record["shares"]:
        assert (sh["V"], sh["nsub"]) == (z["V"], z["nsub"]), (sh, z)
        if z["Mg"] > (20 if z["nsub"] > 1 else 64) * BLOCK:
            return out | {"S5/refused"}  # the solve ends there
        if not sh["exist"]:
            continue  # no shares (sw_share_caps refused): the rows are cleared, nothing placed
        for _, A in sh["A"]:
            out.add(share_form(z["Mg"], z["nsub"], A))
        if z["nsub"] > 1 and z["Mg"] > 8 * BLOCK:
            out.add("S2/nsub>1")
        if z["nsub"] == 1 and z["Mg"] > MERGE_G * CHUNK:  # shares of nsub > 1 are ranked one by one
            out.add("merge>64")
    for pk in record["packs"]:
        assert pk["M"] == z["M"], (pk, z)
        f = gathered_form(pk["M"], pk["A"])
        out.add(f)
        if f == "G7/refused":
            return out
        if pk["M"] > MERGE_G * CHUNK:
            out.add("merge>64")
    for pk in record["share_class_packs"]:  # op_share_repair: this rank's P entries
        # above 64·512 entries (world 1, more than 32,768 jobs) the class's jobs, all
        # inside one share of at most 8,192, go to k_pack_rounds_sel<512,20>
        out.add(gathered_form(z["P"], pk["A"]) if z["P"] <= 64 * BLOCK else "repair>32768")
    rr = record["rr"]
    if rr["words2"]:
        out.add("rr/words>=2")
    if rr["cap512"]:
        out.add("rr/cap>=512")
    if rr["refused_words"]:
        out.add("rr/refused-words")
    if rr["refused_budget"]:
        out.add("rr/refused-budget")
    if rr["refused_capmax"]:
        out.add("rr/refused-capmax")
    return out


ALL_FORMS = frozenset(
    ["S1/wave", "S1/body2", "S1/body4", "S1/body8",
     "S2/wave", "S2/body2", "S2/body4", "S2/body8", "S2/body20", "S2/nsub>1",
     "S3/wave", "S3/sel2", "S3/sel4", "S3/sel8", "S3/rounds32",
     "S4/wave", "S4/sel2", "S4/sel4", "S4/sel8", "S4/rounds64", "S5/refused",
     "G1/wave", "G2/wave", "G2/body2", "G2/body4",
     "G3/body2", "G3/body4", "G3/body8",
     "G4/body2", "G4/body4", "G4/body8", "G4/body20",
     "G5/sel2", "G5/sel4", "G5/sel8", "G5/rounds32",
     "G6/sel2", "G6/sel4", "G6/sel8", "G6/rounds64", "G7/refused",
     "repair>32768", "merge>64", "rr/words>=2", "rr/cap>=512", "rr/refused-words", "rr/refused-budget",
     "rr/refused-capmax"])


# ---- the cases --------------------------------------------------------------
# (name, kind, args).  Chosen on the CPU (DESIGN.md §8 names the form each one
# owns); every instance is a second or two of CPU reference at most.

def _short(name, seed, N, **kw):
    return (name, "short", dict(seed=seed, N=N, k=1e5, **kw))


W357, W16, W1_16, W13 = (3, 5, 7), (1, 2, 4, 8, 16), (1, 1, 1, 1, 1, 16), (1, 1, 1, 2, 2, 13)
W1x12 = (1,) * 12 + (16,)

CASES = (
    # M edges at one share (G = 511, T = 64, unit widths): S1 → S2 → S3 → S4
    [_short(f"edge_N{N}", 1, N) for N in (4096, 4097, 10240, 10241, 16384, 16385, 32768)]
    # every body of the share forms at large M: A set exactly by idle jobs;
    # 512 / 513 the wave hand-over, 4096 / 4097 the one between the two block launches
    + [_short(f"body_N{N}_A{A}", 2, N, idle=N - A)
       for N in (10000, 12000, 20000) for A in (512, 513, 1025, 2049, 4096, 4097)]
    # eight shares above 32,768 jobs (G ≥ 512): trace-shaped, T = 1, T = 64, unit short jobs
    + [("v8_N32769", "synth", dict(seed=21, N=32769, G=2848, T=30, k=1e5)),
       ("v8_N40000", "synth", dict(seed=22, N=40000, G=4096, T=30, k=1e5)),
       ("v8_N65536", "synth", dict(seed=23, N=65536, G=8192, T=30, k=1e5)),
       ("v8_N40000_T1", "synth", dict(seed=25, N=40000, G=3000, T=1, k=1e5)),
       ("v8_repair_N40000_T64", "synth", dict(seed=24, N=40000, G=2048, T=64, k=1e5)),
       _short("v8_short_N40000_T64", 3, 40000, G=512),
       _short("v8_short_N65536_T64", 3, 65536, G=4096)]
    # the gathered ladder: share placements that strand rounds (mixed widths on a
    # cluster a little off their multiples), the orders, raises and class packs after them
    + [_short("gath_N400", 1, 400, G=31, widths=W357),
       _short("gath_N1500", 1, 1500, G=90, widths=W357),
       _short("gath_N3000", 1, 3000, G=509, widths=W13),
       _short("gath_N6000_w357", 1, 6000, G=509, widths=W357),
       _short("gath_N6000_w16", 2, 6000, G=509, widths=W16),
       _short("gath_N6000_w1_16", 1, 6000, G=509, widths=W1_16),
       _short("gath_N12000_w357", 1, 12000, G=509, widths=W357),
       _short("gath_N12000_w16", 1, 12000, G=131, widths=W16),
       _short("gath_N12000_w1_16", 1, 12000, G=509, widths=W1_16),
       _short("gath_N20000_w357", 2, 20000, G=131, widths=W357),
       _short("gath_N20000_w16", 2, 20000, G=509, widths=W16),
       _short("gath_N20000_w1_16", 2, 20000, G=509, widths=W1_16),
       # ... with more active entries than the next smaller variant holds (10,240 / 16,384),
       # and 4,097 / 4,096 of them: the hand-over between the gathered form's two launches
       _short("gath_N14000_A13750", 1, 14000, G=509, widths=W1x12, delta=360.0),
       _short("gath_N24000_A18943", 1, 24000, G=509, widths=(1,) * 16 + (16,), delta=480.0),
       _short("gath_N12000_A4097", 2, 12000, G=300, widths=W1x12, idle=12000 - 4097),
       _short("gath_N20000_A4097", 2, 20000, G=509, widths=W1_16, idle=20000 - 4097),
       _short("gath_N20000_A4096", 2, 20000, G=300, widths=W1x12, idle=20000 - 4097)]
    # fuzz-shaped instances that re-solve (SW_STATUS_P1_REPACKED): class_caps, fill,
    # raises and the pattern step at up to 64 jobs per lane
    + [("fuzz_N5000", "fuzz", dict(seed=300009, N=5000)),
       ("fuzz_N12000", "fuzz", dict(seed=300004, N=12000)),
       ("fuzz_N20000", "fuzz", dict(seed=300002, N=20000)),
       ("fuzz_N32768", "fuzz", dict(seed=300004, N=32768))]
    # the per-round re-optimisation's knapsacks (k_rr; the plan kernel's workspace form)
    + [_short("rr_words2", 1, 2500, G=400, widths=W357),
       _short("rr_cap512", 1, 1100, G=600, widths=(100, 150, 200, 250, 3), idle=800),
       _short("rr_refused_words", 1, 2000, G=250, widths=W357),
       _short("rr_refused_budget", 1, 3000, G=100, widths=W357, idle=1700),
       ("rr_refused_capmax", "short", dict(seed=1, N=2000, G=1100, T=30, k=1e5, widths=(240, 230, 3)))]
)
RR_CASES = [c for c in CASES if c[0].startswith("rr_")]
# share P2 / single-instance P2 above tests/test_shard.py SHARE_P2_RATIO (1.002), measured on
# the CPU engine: a finding about the contract's bar, which was
# measured on trace-shaped instances only — these keep every other assertion
P2_ABOVE_BAR = {"v8_short_N40000_T64": 1.002055}
CASE_IDS = [c[0] for c in CASES]


def worlds(a):
    """The worlds a case runs at: 1 and 2, and 8 where the instance takes
    eight shares."""
    return (1, 2, 8) if share_count(a.N, a.G, 1) == 8 else (1, 2)


# Refusals of the GPU engine (the CPU engine has no such limits): (name, case,
# world, the message).  The placement ones end a solve that the CPU engine
# finishes; include/shockwave_amd.h names the limits.
REFUSALS = [
    ("share_N32769_G511", _short("x", 1, 32769), 1,
     "share placement: a share holds more jobs than one workgroup's round loop"),
    ("eval_N131073", _short("x", 1, 131073, idle=131073 - 600), 1, "eval: more than 256 jobs per lane"),
    ("gathered_N32769_G515", _short("x", 3, 32769, G=515, widths=(1, 2, 4, 8)), 1,
     "sharded placement holds at most 32768 jobs"),
]
