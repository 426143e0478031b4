"""What the host mirrors of the Gavel policies share (policy.py:14-63,
proportional.py:10-44 of the reference, restated once): the flattening of the
``{job_id: {worker_type: value}}`` dictionaries, the reduction of several
identical worker types to one, the [0, 1] clip, and the holder of the native
engine.  A mirror keeps what is its own: its checks and their texts, its
coefficients, its engine call and its ``last_*`` attributes.
"""
import numpy as np

try:
    from . import sw_native
except ImportError:  # flat-module use
    import sw_native


class Policy:
    """The reference's ``name`` property, and the engine of a mirror that keeps
    one in ``_native``: a HIP solver built on first use when none was given."""

    @property
    def name(self):
        return self._name

    def _engine(self):
        if self._native is None:
            self._native = sw_native.Solver(device=0)
        return self._native


def flatten(d):
    """policy.py:28-44: jobs sorted by id, worker types sorted by name (from
    the first job), the throughput matrix; (None, None) without jobs or types."""
    job_ids = sorted(d.keys())
    if len(job_ids) == 0:
        return None, None
    worker_types = sorted(d[job_ids[0]].keys())
    if len(worker_types) == 0:
        return None, None
    m = np.array([[d[j][wt] for wt in worker_types] for j in job_ids], dtype=np.float64)
    return m, (job_ids, worker_types)


def unflatten(x, index):
    job_ids, worker_types = index
    return {job_ids[i]: {worker_types[k]: x[i, k] for k in range(len(worker_types))}
            for i in range(len(job_ids))}


def clipped(x):
    """The reference's ``x.value.clip(min=0.0).clip(max=1.0)``."""
    return x.clip(min=0.0).clip(max=1.0)


def num_workers(worker_types, cluster_spec):
    """The cluster's worker counts in the order of the types, as they are."""
    return [cluster_spec[wt] for wt in worker_types]


def int_workers(worker_types, cluster_spec):
    return [int(cluster_spec[wt]) for wt in worker_types]


def proportional_throughputs(throughputs, worker_types, cluster_spec):
    """ProportionalPolicy.get_throughputs (proportional.py:15-44): the cluster
    split evenly over the jobs, each row scaled to sum to at most 1."""
    m, _ = throughputs.shape
    x = np.array([[cluster_spec[wt] / m for wt in worker_types] for _ in range(m)])
    x = x / np.sum(x, axis=1).max()
    return np.sum(np.multiply(throughputs, x), axis=1)


def identical_types(throughputs):
    """Every job's throughput is the same on every worker type: the program
    sees only Σ_k x[j][k] and one type with Σ workers solves it."""
    return (throughputs == throughputs[:, :1]).all()


def split_over_types(x, workers, total):
    """The one-type shares x_j over the types: x[j][k] = x_j · workers_k / Σ workers,
    which satisfies every type's capacity."""
    m, n = len(x), len(workers)
    if n == 1:
        return x.reshape(m, 1)
    return np.array([[x[i] * workers[k] / total for k in range(n)] for i in range(m)])


def with_v100_throughputs(d):
    """Every worker type's throughput replaced by the job's v100 throughput."""
    return {j: {wt: d[j]["v100"] for wt in d[j]} for j in d}
