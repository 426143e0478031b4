"""bench.py's C5 sub-record: the fixed 512-instance sweep (BASELINE configs[4])
is split over the ranks with the same cluster-size mix on every rank, each
instance solved exactly once (no rank can be left with only the slow small-k
128-GPU configuration).  And its command line: a plain run prints the
headline line only, --dump-outputs writes the last timed step's results."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import sw_synth as ss  # noqa: E402


def test_sweep_cycles_cluster_sizes():
    probs = ss.sweep_problems(8, N=12)
    assert [p.G for p in probs] == [32, 64, 128, 256] * 2
    assert all(p.T == 30 for p in probs)
    k = {p.G: p.k for p in probs}
    assert k == {32: 10.0, 64: 10.0, 128: 1e-3, 256: 1e5}


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_c5_share_same_mix_every_rank(world):
    sizes = (32, 64, 128, 256)
    idx = list(range(bench.C5_INSTANCES))
    seen = []
    for rank in range(world):
        mine = bench.c5_share(idx, world, rank)
        seen += mine
        mix = collections.Counter(sizes[i % 4] for i in mine)
        assert mix == {G: bench.C5_INSTANCES // 4 // world for G in sizes}, (world, rank, mix)
    assert sorted(seen) == idx


def _fake_results(n, N=9, T=5):
    rng = np.random.default_rng(3)
    return [dict(plan=rng.integers(0, 2, (N, T)).astype(np.uint8),
                 planned_rounds=rng.integers(0, T + 1, N).astype(np.int32),
                 objective=-1.5 * i, utility=0.25 * i, makespan=7.0, p2_objective=2.0 * i,
                 bound=-1.0 * i, iters=20 + i, status=i % 3) for i in range(n)]


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    res = _fake_results(40)
    per = 4 * 9 * 5 + 4 * 9
    monkeypatch.setattr(bench, "DUMP_BYTES", 7 * per + 1)  # room for 7 of the 40 instances
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(k + ".npy" for k in (
        "objective", "utility", "makespan", "p2_objective", "bound", "iters", "status",
        "sample_instances", "plan", "planned_rounds"))
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:  # the same inputs give the same files, sample included
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n)), n
        assert a[n].dtype in (np.float32, np.float64), n
    pick = a["sample_instances.npy"].astype(int)
    assert len(pick) == 7 and len(set(pick)) == 7 and list(pick) == sorted(pick)
    assert a["plan.npy"].shape == (7, 9, 5) and a["planned_rounds.npy"].shape == (7, 9)
    for s, i in enumerate(pick):
        assert np.array_equal(a["plan.npy"][s], res[i]["plan"])
        assert np.array_equal(a["planned_rounds.npy"][s], res[i]["planned_rounds"])
    assert np.array_equal(a["objective.npy"], [r["objective"] for r in res])
    assert np.array_equal(a["iters.npy"], [r["iters"] for r in res])
    # everything is kept when it fits
    monkeypatch.setattr(bench, "DUMP_BYTES", 40 * per)
    bench.dump_outputs(str(tmp_path / "c"), res)
    assert np.array_equal(np.load(tmp_path / "c" / "sample_instances.npy"), np.arange(40))


def test_full_and_dump_are_off_unless_asked_for(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--no-c4"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.no_c4 and a.cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_default_dump_stays_under_64_mb():
    # default batch: the sampled per-job arrays plus seven float64 scalars per instance
    assert bench.DUMP_BYTES + 32768 * 7 * 8 + 11 * 4096 < 64_000_000


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path, gpu_solver):
    """A plain run times exactly --steps steps, prints one line with the
    headline fields and none of the --full sub-records, and --dump-outputs
    holds what the device-resident path computed: bit for bit what a solve of
    the same seeded instances returns."""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--batch", "48", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "plan-solves/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(48 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("cpu_baseline", "c5_sweep", "c4_sharded", "single_instance_ms", "onchip",
                "host_boundary_solves_per_s", "sustained_solves_per_s"):
        assert key not in line, key
    batch = [ss.synth_problem(i, 900, 256, 30, 120.0, 1e5, 5.0) for i in range(48)]
    want = gpu_solver.solve_batch(batch)
    assert np.array_equal(np.load(out / "sample_instances.npy"), np.arange(48))
    assert np.array_equal(np.load(out / "plan.npy"), np.stack([r["plan"] for r in want]))
    assert np.array_equal(np.load(out / "planned_rounds.npy"),
                          np.stack([r["planned_rounds"] for r in want]))
    for key in ("objective", "utility", "makespan", "p2_objective", "bound", "iters", "status"):
        got = np.load(out / (key + ".npy"))
        assert got.dtype == np.float64
        assert got.tobytes() == np.array([r[key] for r in want], dtype=np.float64).tobytes(), key


def test_c5_order_puts_small_k_first_and_keeps_every_instance():
    probs = bench.c5_share(ss.sweep_problems(64, N=12), 2, 1)
    ordered = bench.c5_order(probs)
    assert sorted(id(p) for p in ordered) == sorted(id(p) for p in probs)
    ks = [p.k for p in ordered]
    assert ks == sorted(ks) and ks[0] == 1e-3
