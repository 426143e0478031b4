"""Case generators for the P2 exchange step's own tests (tests/test_p2x.py on
the CPU, tests/test_gpu_p2x.py on the GPU): synthetic round graphs for
find_cycle and feasible placements that no placement cascade produced.

A graph case is (T, F, W[T][T], room[T]) with small-integer costs, so every
sum of costs is exact in doubles.  A placement is a dict with T, G, job, w, c,
m (round masks as Python ints); see p2x_ref.py.
"""
import numpy as np

import p2x_ref as pr

GRAPH_T = (2, 3, 5, 17, 31, 32, 33, 63, 64)
NONE = pr.NONE


# ---- graphs ---------------------------------------------------------------

def _graph(T, F, W, room):
    W = np.array(W, dtype=np.float64).reshape(T, T)
    for t in range(T):
        W[t, t] = NONE
    return T, int(F), W, [int(x) for x in room]


def random_graph(rng, T):
    """Integer costs at a random density, biased so that roughly half of the
    graphs have a negative cycle; some with free capacity (edges into V)."""
    kind = rng.integers(0, 4)
    p = (0.08, 0.3, 1.0)[rng.integers(0, 3)] if T > 3 else (0.5, 1.0)[rng.integers(0, 2)]
    if kind == 0:  # reduced costs r + π(u) − π(t), r ≥ 0: no negative cycle, many zero-cost ones
        pi = rng.integers(-6, 7, size=T)
        W = rng.integers(0, 4, size=(T, T)) + pi[None, :] - pi[:, None]
    elif kind == 1:  # the same with a few entries lowered: a few short negative cycles, or none
        pi = rng.integers(-6, 7, size=T)
        W = rng.integers(0, 4, size=(T, T)) + pi[None, :] - pi[:, None]
        for _ in range(rng.integers(1, 4)):
            W[rng.integers(0, T), rng.integers(0, T)] -= rng.integers(1, 4)
    else:
        lo = (-1, 0, -3)[rng.integers(0, 3)]
        W = rng.integers(lo, (4, 9, 30)[rng.integers(0, 3)], size=(T, T))
    W = W.astype(np.float64)
    W[rng.random((T, T)) >= p] = NONE
    F = int(rng.integers(1, 5))
    room = rng.integers(0, 2 * F + 1, size=T) if rng.random() < 0.5 else np.zeros(T, dtype=np.int64)
    return _graph(T, F, W, room)


def perturb_rows(rng, g):
    """The graph with two rows redrawn (what a cancel does to W, roughly)."""
    T, F, W, room = g
    W = W.copy()
    for t in rng.choice(T, size=min(2, T), replace=False):
        row = rng.integers(-2, 8, size=T).astype(np.float64)
        row[rng.random(T) >= 0.5] = NONE
        W[t] = row
    return _graph(T, F, W, room)


def random_graphs(seed=5, per_t=None):
    """[(cold graph, perturbed graph)] over GRAPH_T."""
    rng = np.random.default_rng(seed)
    out = []
    for T in GRAPH_T:
        n = per_t if per_t is not None else (60 if T <= 33 else 24)
        for _ in range(n):
            g = random_graph(rng, T)
            out.append((g, perturb_rows(rng, g)))
    return out


def ring(T, through_v=False, cost=-1.0):
    """0 → 1 → … → T−1 → 0 (each edge at cost), or closed T−1 → V → 0 through
    the free-capacity node: the only cycle, of T or T + 1 nodes."""
    W = np.full((T, T), NONE)
    for t in range(T - 1):
        W[t, t + 1] = cost
    room = [0] * T
    if through_v:
        room[T - 1] = 1
    else:
        W[T - 1, 0] = cost
    return _graph(T, 1, W, room)


def tie_graphs():
    """Named graphs for the tie rules: first predecessor wins, zero-cost and
    −0.0 cycles are not negative, no edges at all."""
    out = {}
    for T in (2, 3, 5, 33, 64):
        W = np.full((T, T), NONE)
        out[f"no_edges_T{T}"] = _graph(T, 1, W, [0] * T)
        out[f"no_edges_room_T{T}"] = _graph(T, 1, W, [1] * T)
        out[f"all_zero_T{T}"] = _graph(T, 1, np.zeros((T, T)), [0] * T)
        out[f"all_minus_zero_T{T}"] = _graph(T, 1, np.full((T, T), -0.0), [1] * T)
        out[f"all_equal_negative_T{T}"] = _graph(T, 1, np.full((T, T), -1.0), [0] * T)
        out[f"all_equal_negative_room_T{T}"] = _graph(T, 2, np.full((T, T), -1.0), [2] * T)
        # zero-cost ring: +1 … +1 and one edge −(T − 1)
        g = ring(T, cost=1.0)
        g[2][T - 1, 0] = -(T - 1.0)
        out[f"zero_ring_T{T}"] = g
        g = ring(T, cost=1.0)
        g[2][T - 1, 0] = -(T - 1.0) - 1.0
        out[f"minus_one_ring_T{T}"] = g
        if T >= 3:
            # equal-cost predecessors of every node: two parallel rings (step 1 and step 2)
            W = np.full((T, T), NONE)
            for t in range(T):
                W[t, (t + 1) % T] = -1.0
                W[t, (t + 2) % T] = -1.0
            out[f"two_rings_T{T}"] = _graph(T, 1, W, [0] * T)
            # every node reached at equal cost from round 0, from V and from its neighbour
            W = np.full((T, T), NONE)
            for u in range(1, T):
                W[0, u] = -2.0
                W[u - 1, u] = -2.0 if u > 1 else -2.0
            W[T - 1, 0] = 1.0
            out[f"equal_preds_T{T}"] = _graph(T, 1, W, [1] + [0] * (T - 1))
    return out


# ---- placements -----------------------------------------------------------

def c_values(rng, A, kind):
    if kind == "uniform":
        return rng.uniform(0.05, 10.0, size=A)
    if kind == "ratio":  # priorities over counts, like p/n
        return rng.integers(1, 9, size=A) / rng.integers(1, 33, size=A)
    if kind == "few":  # many equal values: order falls to the job id
        return rng.choice(np.array([0.25, 0.5, 1.0, 1.5]), size=A)
    if kind == "equal":
        return np.full(A, 0.75)
    if kind == "zero":
        return np.zeros(A)
    if kind == "some_zero":
        c = rng.uniform(0.05, 10.0, size=A)
        c[rng.random(A) < 0.3] = 0.0
        return c
    if kind == "low_bits":  # pairs that differ only in the 3 mantissa bits the rank key drops
        base = rng.choice(rng.uniform(0.5, 4.0, size=max(1, A // 3)), size=A)
        bits = base.view(np.uint64) & ~np.uint64(7) | rng.integers(0, 8, size=A).astype(np.uint64)
        return bits.view(np.float64)
    if kind == "wide":  # 1e-300 … 1e295: costs stay under the 1e300 no-edge value
        return 10.0 ** rng.uniform(-300, 295, size=A)
    if kind == "sentinel":  # at and above the no-edge value
        c = 10.0 ** rng.uniform(296, 303, size=A)
        c[: max(1, A // 4)] = NONE
        return c
    raise ValueError(kind)


def placement(rng, T, w, G, cdist="uniform", fill=1.0, job_step=1):
    """A feasible placement of the jobs of widths w on T rounds of G GPUs:
    every round takes jobs, fewest rounds so far first (random among equals),
    while its load stays ≤ fill·G — so with width-1 jobs to spare the rounds at
    fill 1 are saturated exactly.  Every job is active (≥ 1 round); the
    generator raises if G is too small for that.  fill may be a per-round list."""
    w = np.array(w, dtype=np.int64)
    A = len(w)
    m = [0] * A
    cnt = np.zeros(A, dtype=np.int64)
    fills = [fill] * T if np.isscalar(fill) else list(fill)
    for t in rng.permutation(T):
        cap = int(G * fills[t])
        load = 0
        for i in np.lexsort((rng.random(A), cnt)):
            if load + w[i] <= cap:
                load += int(w[i])
                m[i] |= 1 << int(t)
                cnt[i] += 1
                if load == cap:
                    break
    if A and cnt.min() == 0:
        raise ValueError("placement: G too small for every job to be active")
    job = (np.arange(A) * job_step + (3 if job_step > 1 else 0)).astype(np.int64)
    return dict(T=int(T), G=int(G), job=[int(x) for x in job], w=[int(x) for x in w],
                c=[float(x) for x in c_values(rng, A, cdist)], m=m)


def tidied(P):
    """The placement's jobs and counts placed again, largest c per GPU first, each job
    in the earliest rounds that still have room: near the optimum, so the step
    needs few cancels.  A job keeps at least one round or the result is None."""
    T, G, w, c = P["T"], P["G"], P["w"], P["c"]
    load = [0] * T
    m = [0] * len(w)
    for i in sorted(range(len(w)), key=lambda i: -c[i] / w[i]):
        need = bin(P["m"][i]).count("1")
        for t in range(T):
            if need and load[t] + w[i] <= G:
                load[t] += w[i]
                m[i] |= 1 << t
                need -= 1
        if m[i] == 0:
            return None
    return dict(P, m=m)


def shuffle_rounds(rng, P, moves):
    """The placement after random feasible single-job moves (keeps counts and
    loads ≤ G): what the generator's fewest-first rule would never leave."""
    T, G, w, m = P["T"], P["G"], P["w"], list(P["m"])
    load = pr.loads(T, w, m)
    A = len(w)
    for _ in range(moves):
        i = int(rng.integers(0, A))
        ins = [t for t in range(T) if (m[i] >> t) & 1]
        outs = [t for t in range(T) if not (m[i] >> t) & 1 and load[t] + w[i] <= G]
        if not ins or not outs:
            continue
        t, u = ins[rng.integers(0, len(ins))], outs[rng.integers(0, len(outs))]
        m[i] ^= (1 << t) | (1 << u)
        load[t] -= w[i]
        load[u] += w[i]
    return dict(P, m=m)


def widths_of(sizes):
    """[w per job] from {width: jobs}, interleaved so classes share the id range."""
    out = []
    for wk, n in sizes.items():
        out += [wk] * n
    return out


WIDTH_SETS = {
    "w1": (1,),
    "w1248": (1, 2, 4, 8),
    "w136": (1, 3, 6),
    "w2_255": (2, 255),
    "eight": (1, 2, 3, 4, 5, 6, 8, 12),
}


def random_placements(n, seed, max_a=200, max_t=32, cdists=("uniform", "ratio", "few"), single=False):
    """n random feasible placements: A ≤ max_a, T ≤ max_t, a width set, a c
    distribution, saturated or with room, then shuffled."""
    rng = np.random.default_rng(seed)
    out = []
    names = ["w1"] if single else ["w1", "w1", "w1248", "w136", "eight", "w1248", "w2_4"]
    while len(out) < n:
        name = names[rng.integers(0, len(names))]
        ws = (2, 4) if name == "w2_4" else WIDTH_SETS[name]
        A = int(rng.integers(2, max_a + 1))
        T = int(rng.integers(2, max_t + 1))
        pw = np.array([1.0 / (1 + k) for k in range(len(ws))])
        w = rng.choice(np.array(ws), size=A, p=pw / pw.sum())
        if single:
            w[:] = int(rng.choice(np.array([1, 1, 2, 4])))
        w[0] = ws[0] if not single else w[0]
        per_round = int(w.sum()) * float(rng.uniform(1.1, 4.0)) / T
        G = max(int(w.max()), int(np.ceil(per_round)))
        if single:
            G = max(int(w[0]), G // int(w[0]) * int(w[0]))
        fill = 1.0 if rng.random() < 0.5 else [float(x) for x in rng.uniform(0.6, 1.0, size=T)]
        # large instances mostly start near their optimum: far from it they stop at the cancel cap
        tidy = A > 80 and rng.random() < 0.9
        try:
            P = placement(rng, T, w, G, cdists[rng.integers(0, len(cdists))], fill)
        except ValueError:
            continue
        P = tidied(P) if tidy else P
        if P is None:
            continue
        out.append(shuffle_rounds(rng, P, int(rng.integers(0, A // 8 if tidy else 3 * A))))
    return out


def room_threshold_case(rng, T, sizes, F, cdist="uniform"):
    """Saturated exactly, then one round left with room exactly F (a width-F
    job taken out) and another with room exactly F − 1 (a width-F job taken
    out, a width-1 job put in): the t → V threshold on both sides."""
    w = widths_of(sizes)
    A = len(w)
    G = int(np.ceil(sum(w) * 2.0 / T))
    G = max(G, max(w))
    P = placement(rng, T, w, G, cdist)
    m, ld = list(P["m"]), pr.loads(T, w, P["m"])
    sat = [t for t in range(T) if ld[t] == G]
    done = 0
    for t in sat:
        if done == 2:
            break
        out = [i for i in range(A) if w[i] == F and (m[i] >> t) & 1 and bin(m[i]).count("1") >= 2]
        if not out:
            continue
        if done == 1 and F >= 2:
            add = [i for i in range(A) if w[i] == 1 and not (m[i] >> t) & 1]
            if not add:
                continue
            m[add[0]] |= 1 << t
        m[out[0]] &= ~(1 << t)
        done += 1
    if done < 2:
        raise ValueError("room_threshold_case: no saturated round with a width-F job to take out")
    return dict(P, m=m)


def shape_cases():
    """The shapes at which the device code takes another path, by name."""
    rng = np.random.default_rng(20)
    out = {}
    # T at the wave edge, one class, M across the 64-rank word edge
    for T in (2, 3, 31, 32, 33, 63, 64):
        for M in (1, 63, 64, 65, 128, 129):
            if T in (3, 31, 33, 63) and M in (63, 128):
                continue  # the word edge itself is covered at the other T
            G = max(1, int(np.ceil(M * 1.5 / T)))
            P = placement(rng, T, [1] * M, G, "uniform" if M % 2 else "few")
            out[f"T{T}_M{M}"] = shuffle_rounds(rng, P, 2 * M)
    # A across the register sort / LDS sort edge, the power-of-two padding and AMAX, T = 8
    for A in (1, 2, 511, 512, 513, 1024, 1025, 4096, 4097):
        w = [1] * A if A < 511 else list(rng.choice(np.array([1, 1, 1, 2, 4]), size=A))
        G = max(max(w), int(np.ceil(sum(w) * 1.5 / 8)))
        P = placement(rng, 8, w, G, "ratio", job_step=3 if A == 513 else 1)
        out[f"A{A}_T8"] = shuffle_rounds(rng, P, A)
    # width sets: q = 2 and 4, 8/1 excluded by QMAX; {1, 3, 6}; {2, 255}; eight and nine classes
    out["w1248_T16"] = shuffle_rounds(rng, placement(rng, 16, widths_of({1: 70, 2: 40, 4: 20, 8: 9}), 48), 150)
    out["w1248_T64"] = shuffle_rounds(rng, placement(rng, 64, widths_of({1: 130, 2: 66, 4: 30, 8: 12}), 24), 300)
    out["w136_T12"] = shuffle_rounds(rng, placement(rng, 12, widths_of({1: 40, 3: 30, 6: 12}), 36), 100)
    out["w2_255_T6"] = shuffle_rounds(rng, placement(rng, 6, widths_of({2: 140, 255: 5}), 510), 100)
    out["eight_classes_T10"] = shuffle_rounds(
        rng, placement(rng, 10, widths_of({x: 12 for x in WIDTH_SETS["eight"]}), 130), 100)
    out["nine_classes_T10"] = placement(rng, 10, widths_of({x: 8 for x in (1, 2, 3, 4, 5, 6, 8, 12, 16)}), 160)
    # G: saturated exactly, and room exactly F and F − 1
    out["saturated_w1_T32"] = placement(rng, 32, [1] * 100, 10, "uniform")
    out["saturated_w1248_T31"] = placement(rng, 31, widths_of({1: 90, 2: 30, 4: 12, 8: 6}), 24, "ratio")
    for F in (1, 2, 4, 8):
        out[f"room_F{F}_T9"] = room_threshold_case(rng, 9, {1: 40, 2: 16, 4: 8, 8: 4}, F)
    out["room_F1_T64"] = room_threshold_case(rng, 64, {1: 129}, 1)
    # c
    sizes = {1: 65, 2: 20, 4: 8}
    for cd in ("equal", "low_bits", "zero", "some_zero", "wide"):
        P = placement(rng, 12, widths_of(sizes), 20, cd, [0.8] * 6 + [1.0] * 6)
        out[f"c_{cd}"] = shuffle_rounds(rng, P, 200)
    # long cycles (found by a search; lengths measured with an instrumented twin): one job per
    # round at G = 1 with c a rotated geometric sequence, so a rotation of many rounds is the first
    # cycle Bellman–Ford closes — 14 nodes at T = 20, 23 at T = 63; and round 0 empty at T = 64,
    # where the cancels shift chains of jobs one round down through V (13 nodes)
    out["long_cycle_T20"] = rotated_geometric(20, 0.5, 17)
    out["long_cycle_T63"] = rotated_geometric(63, 0.8, 51)
    out["long_cycle_V_T64"] = dict(T=64, G=1, job=list(range(63)), w=[1] * 63,
                                   c=[float(0.8 ** u) for u in range(1, 64)], m=[1 << u for u in range(1, 64)])
    # edges of q = 2 and 4 jobs out of a class of three and four rank words: the selection
    # (first pick, then the next picks) runs across the 64-rank word edges
    rng2 = np.random.default_rng(23)
    out["w124_M200_T8"] = shuffle_rounds(rng2, placement(rng2, 8, widths_of({1: 200, 2: 30, 4: 10}), 80), 300)
    out["w12_M250_T5"] = shuffle_rounds(rng2, placement(rng2, 5, widths_of({1: 250, 2: 20}), 120, "few"), 300)
    return out


def rotated_geometric(T, r, shift):
    """Job u alone in round u (G = 1, saturated), c_u = r^((u + shift) mod T)."""
    return dict(T=T, G=1, job=list(range(T)), w=[1] * T, c=[float(r ** ((u + shift) % T)) for u in range(T)],
                m=[1 << u for u in range(T)])


def sentinel_case():
    """c at and above the no-edge value: held to twin equality and the invariants only."""
    rng = np.random.default_rng(21)
    P = placement(rng, 12, widths_of({1: 65, 2: 20, 4: 8}), 20, "sentinel", [0.8] * 6 + [1.0] * 6)
    return shuffle_rounds(rng, P, 200)


def skip_cases():
    """Placements the step must leave alone: A > 4096, K > 8, T < 2, A = 0."""
    sc = shape_cases()
    rng = np.random.default_rng(22)
    one_round = dict(T=1, G=8, job=list(range(8)), w=[1] * 8, c=[float(x) for x in rng.uniform(1, 2, 8)],
                     m=[1] * 8)
    empty = dict(T=8, G=4, job=[], w=[], c=[], m=[])
    return {"A4097": sc["A4097_T8"], "nine_classes": sc["nine_classes_T10"], "T1": one_round, "A0": empty}
