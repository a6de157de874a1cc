"""CPU tests of bench.py's --dump-outputs writer (dump_outputs) on a stand-in filter with the headline's array shapes."""
import os

import numpy as np

import bench


class _Filter:
    """What ParticleFilter hands back after a sweep, at the sizes of the default workload (100 Mb, Np = 10 000, 4 haplotypes)."""

    def __init__(self, rows=186024, bins=1000000, Np=10000, n=4):
        self.rows, self.bins, self.Np, self.n = rows, bins, Np, n

    def trace(self):
        r = self.rows
        return {"T": np.arange(r) * 537.0, "ess": np.random.default_rng(1).random(r), "resampled": np.zeros(r, np.int32), "logl": -np.arange(r) * 9.0}

    def local_recomb(self):
        rng = np.random.default_rng(2)
        return {"opp_diff": rng.standard_normal(self.bins), "counts": rng.random((self.n + 2, self.bins))}

    def particles(self):
        Np, n = self.Np, self.n
        return {"w_post": np.ones(Np), "w_pilot": np.ones(Np), "heights": np.random.default_rng(3).random((Np, n - 1)),
                "children": np.ones((Np, n - 1, 2), np.int8), "next_base": np.zeros(Np)}


def _dump(path, f):
    counts = {"coal_count": np.arange(32.0), "delayed_opp": 1.5, "logl": -12.5}
    bench.dump_outputs(str(path), [(f, None)], -12.5, counts, local_recomb=True)
    return {name[:-4]: np.load(os.path.join(path, name)) for name in sorted(os.listdir(path))}


def test_dump_outputs_float64_within_budget_and_sampled_the_same_way(tmp_path):
    a = _dump(tmp_path / "a", _Filter())
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert a["logl"].tolist() == [-12.5] and a["counts_delayed_opp"].tolist() == [1.5]
    assert a["trace_T"].shape == (186024,) and a["particles_children"].shape == (10000, 3, 2)
    # 6 x 1e6 values do not fit: a sample, with its flat indices beside it
    idx = a["local_recomb_counts_index"].astype(np.int64)
    assert len(idx) == len(a["local_recomb_counts"]) < 6 * 1000000 and (np.diff(idx) > 0).all()
    full = _Filter().local_recomb()["counts"].reshape(-1)
    np.testing.assert_array_equal(a["local_recomb_counts"], full[idx])
    b = _dump(tmp_path / "b", _Filter())
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_outputs_shrinks_the_sample_until_everything_fits(tmp_path):
    a = _dump(tmp_path / "big", _Filter(rows=3000000, bins=3000000))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert "trace_T_index" in a and "local_recomb_opp_diff_index" in a
