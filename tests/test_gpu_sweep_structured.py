"""Chunks of structured models in lockstep (pf_run_many on the register-tree row pipeline: one k_sweep_xmp launch and one
k_sweep_blc launch per row for all chunks).  Every chunk must be bit-identical to its own pf_run and to the oracle, whatever
the calls are cut into, whoever leads, and whatever runs on a handle in between; groups the launches cannot serve are refused."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

import cases
from smcsmc_amd import ParticleFilter, PfError

pytestmark = pytest.mark.gpu

FRACTIONS = (0.5, 0.7, 0.85, 1.0)
CASES = [(8, 2, 640, False), (6, 3, 500, False), (4, 2, 512, True), (4, 4, 200, False)]
HEAD = (8, 2, 640, False)
CALL = 29


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _chunks(n, P, biased):
    """four chunks of one model: lengths 0.5, 0.7, 0.85 and 1.0 x 1.2e5, each with its own data"""
    out = []
    for k, frac in enumerate(FRACTIONS):
        base = cases.make_model(n=n, E=8, L=1.2e5 * frac)
        segs = cases.make_segments(base, seed=50 + 10 * n + 3 * k, max_seg_len=4000)
        model = cases.make_structured(base, P=P, split_epoch=5, mig=1.5)
        if biased:
            model = dict(model, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(8, 2500.0), delay_type=0)
        out.append((model, segs))
    return out


def _new(model, segs, Np, seed, **kw):
    f = ParticleFilter(model, Np, seed=seed, local_recomb=True, **kw)
    f.init_prior(0.0); f.load_segments(segs)
    return f


def _snap(f):
    """everything the comparisons read, so that the filter itself can go"""
    s, p = f.resample_events()
    return dict(logl=f.logl(), trace=f.trace(), rs=(s, p), counts=f.counts(), particles=f.particles(), mig=f.migrations(),
                lmap=f.local_recomb(), done=f.segments_done(), rows=f.n_segs)


@functools.lru_cache(maxsize=None)
def _alone(n, P, Np, biased, count_wgs=0):
    """pf_run of every chunk on its own, computed once per shape and left unchanged"""
    out = []
    for k, (m, sg) in enumerate(_chunks(n, P, biased)):
        f = _new(m, sg, Np, 3 + k, count_wgs=count_wgs)
        f.run(); f.finish()
        out.append(_snap(f))
        f.close()
    return out


def _group(n, P, Np, biased, count_wgs=0):
    return [_new(m, sg, Np, 3 + k, count_wgs=count_wgs) for k, (m, sg) in enumerate(_chunks(n, P, biased))]


def _lockstep(many, call):
    nmax = max(f.n_segs for f in many)
    for s0 in range(0, nmax, call):                         # chunks that are done sit the later calls out
        ParticleFilter.run_many(many, s0, min(nmax, s0 + call))
    for f in many:
        f.finish()


def _same(a, b):
    """a, b: snapshots.  Log-likelihood, traces, resampling, counts, particles and migration events bit for bit; the local
    recombination map (atomics: same terms, any order) by the rule of test_gpu_sweep.py"""
    assert a["done"] == b["done"]
    assert _bits(a["logl"]) == _bits(b["logl"])
    for k in ("T", "ess", "logl"):
        assert (_bits(a["trace"][k]) == _bits(b["trace"][k])).all(), k
    assert (a["trace"]["resampled"] == b["trace"]["resampled"]).all()
    assert (a["rs"][0] == b["rs"][0]).all() and (a["rs"][1] == b["rs"][1]).all()
    for k in a["counts"]:
        assert (_bits(a["counts"][k]) == _bits(b["counts"][k])).all(), k
    for k in a["particles"]:
        assert (np.asarray(a["particles"][k]).view(np.uint8) == np.asarray(b["particles"][k]).view(np.uint8)).all(), k
    for k in a["mig"]:
        x, y = np.asarray(a["mig"][k]), np.asarray(b["mig"][k])
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), k
    for k in a["lmap"]:
        ref = np.asarray(b["lmap"][k], dtype=np.float64)
        np.testing.assert_allclose(a["lmap"][k], ref, rtol=1e-9, atol=1e-12 * max(1e-300, float(np.abs(ref).max())), err_msg=k)


def _all_same(many, alone):
    for f, g in zip(many, alone):
        _same(_snap(f), g)


@pytest.mark.parametrize("n,P,Np,biased", CASES)
def test_structured_chunks_in_lockstep_equal_their_own_runs(hiplib, n, P, Np, biased):
    """Four chunks with their own data, lengths and seeds through pf_run_many in calls of 29 rows (a finished chunk sits the later
    calls out, every call re-seeds the window state): each equals its pf_run.  Np = 500 and 200 leave the last extend workgroup
    partly filled; P = 4 is the PF_PMAX instance of the count kernels."""
    alone = _alone(n, P, Np, biased)
    many = _group(n, P, Np, biased)
    assert ParticleFilter.can_run_many(many)
    assert len({f.n_segs for f in many}) == len(many)                       # the chunks end at different rows
    assert min(f.n_segs for f in many) >= 40                                # the sixteen-slot rings wrap, the every-eighth-step wait is reached
    _lockstep(many, CALL)
    for f in many:
        assert int(f.trace()["resampled"].sum()) >= 3
    assert any(int(np.asarray(f.migrations()["n_events"]).sum()) > 0 for f in many)
    _all_same(many, alone)


def _canon_events(mg):
    out = []
    for i in range(len(mg["n_events"])):
        k = mg["n_events"][i]
        out.append(sorted(zip(_bits(mg["times"][i, :k]).tolist(), mg["branch"][i, :k].tolist(), mg["newpop"][i, :k].tolist())))
    return out


def test_a_chunk_of_the_lockstep_run_equals_the_oracle(oracle, hiplib):
    """Chunk 1 of the (8, 2, 640) group: log-likelihood, resampling parents, final trees, node populations and migration events
    bit for bit the oracle's; the counts, migration statistics included, to 1e-9 (sums in another order)."""
    n, P, Np, biased = HEAD
    many = _group(n, P, Np, biased)
    _lockstep(many, CALL)
    model, segs = _chunks(n, P, biased)[1]
    g = many[1]
    o = oracle.Oracle(model, Np, seed=3 + 1)
    o.init_prior(0.0); o.run(o.pack_segments(model, segs))
    assert _bits(g.logl()) == _bits(o.logl())
    so, po_ = o.resample_events(); sg, pg_ = g.resample_events()
    assert len(so) >= 3 and (so == sg).all() and (po_ == pg_).all()
    po, pg = o.particles(), g.particles()
    assert (po["children"] == pg["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(po[k]) == _bits(pg[k])).all(), k
    mo, mg = o.migrations(), g.migrations()
    assert (mo["n_events"] == mg["n_events"]).all()
    assert (mo["node_pops"] == mg["node_pops"]).all()
    assert _canon_events(mo) == _canon_events(mg)
    co, cg = o.counts(), g.counts()
    assert co["mig_count"].sum() > 0
    for k in ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight", "mig_count", "mig_opp", "mig_weight"):
        np.testing.assert_allclose(cg[k], co[k], rtol=1e-9, atol=1e-300, err_msg=k)
    assert cg["resample_count"] == co["resample_count"]


def test_one_call_over_all_rows_equals_the_calls_of_29_rows(hiplib):
    n, P, Np, biased = HEAD
    alone = _alone(n, P, Np, biased)               # = the calls of 29 rows (the first test)
    one = _group(n, P, Np, biased)
    ParticleFilter.run_many(one)
    for f in one:
        f.finish()
    cut = _group(n, P, Np, biased)
    _lockstep(cut, CALL)
    for f, g, ref in zip(one, cut, alone):
        _same(_snap(f), _snap(g))
        _same(_snap(f), ref)


def test_tapered_count_columns_in_lockstep(hiplib):
    """count_wgs = 2 on both sides: the tapered columns and the trimmed ledger width, lockstep against the runs alone"""
    n, P, Np, biased = HEAD
    alone = _alone(n, P, Np, biased, 2)
    many = _group(n, P, Np, biased, 2)
    assert ParticleFilter.can_run_many(many)
    _lockstep(many, CALL)
    _all_same(many, alone)


def test_a_run_alone_between_two_lockstep_calls(hiplib):
    """60 rows of all chunks in lockstep, the next 10 rows of one chunk by pf_run on its own handle and stream (the others take
    theirs in lockstep without it, under the same leader), then the rest together: the straight run of every chunk."""
    n, P, Np, biased = HEAD
    alone = _alone(n, P, Np, biased)
    many = _group(n, P, Np, biased)
    nmax = max(f.n_segs for f in many)
    assert min(f.n_segs for f in many) > 70
    ParticleFilter.run_many(many, 0, 60)
    many[2].run(60, 70)
    ParticleFilter.run_many([f for k, f in enumerate(many) if k != 2], 60, 70)
    ParticleFilter.run_many(many, 70, nmax)
    for f in many:
        f.finish()
    _all_same(many, alone)


def _refused(group):
    assert not ParticleFilter.can_run_many(group)
    with pytest.raises(PfError, match="pf_run_many"):
        ParticleFilter.run_many(group)


def test_groups_the_structured_launches_cannot_serve_are_refused(hiplib):
    from smcsmc_amd import pf, segments as segmod
    base = cases.make_model(n=4, E=6, L=4e4)
    segs = cases.make_segments(base, seed=2, max_seg_len=4000)
    m2 = cases.make_structured(base, P=2, split_epoch=4, mig=1.5)
    m3 = cases.make_structured(base, P=3, split_epoch=4, mig=1.5)
    a, b = _new(m2, segs, 256, 1), _new(m2, segs, 256, 2)
    assert ParticleFilter.can_run_many([a, b]) and ParticleFilter.can_run_many([b])
    with pytest.raises(PfError, match="twice"):
        ParticleFilter.run_many([a, a])
    # the LDS tree (more than 8 haplotypes)
    b12 = cases.make_model(n=12, E=6, L=4e4)
    s12 = cases.make_segments(b12, seed=2, max_seg_len=4000)
    m12 = cases.make_structured(b12, P=2, split_epoch=4, mig=1.5)
    _refused([_new(m12, s12, 256, 1), _new(m12, s12, 256, 2)])
    # the auxiliary particle filter
    rows = [(int(s) + 1, int(l), int(st), list(map(int, al)))
            for s, l, st, al in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    la = segmod.pack_lookahead(rows, 4)
    tbl = pf.terminal_branch_quantiles(m2, seed=1, n_trees=4000)
    c, d = _new(m2, segs, 256, 3), _new(m2, segs, 256, 4)
    c.load_lookahead(la, 2, tbl); d.load_lookahead(la, 2, tbl)
    _refused([c, d])
    _refused([a, c])
    # chunks that do not share what the launches take from the leader
    with pytest.raises(PfError, match="must share"):
        ParticleFilter.run_many([a, _new(m3, segs, 256, 2)])
    assert not ParticleFilter.can_run_many([a, _new(m3, segs, 256, 2)])
    with pytest.raises(PfError, match="must share"):
        ParticleFilter.run_many([a, _new(m2, segs, 256, 2, mig_cap=64)])
    assert not ParticleFilter.can_run_many([a, _new(m2, segs, 256, 2, mig_cap=64)])
    one_pop = _new(base, segs, 256, 2)
    _refused([a, one_pop])
    _refused([one_pop, a])


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binary_structured_chunks_do_not_depend_on_the_ranks(hiplib, built_binary, tmp_path):
    """bin/smcsmc -chunks 3 on the two-population data of test_structured_binary_end_to_end: one rank with three chunks and three
    ranks with a chunk each give the same .out, byte for byte, and the same maps.  The binary filters the chunks of a structured
    model one after the other (lockstep has not been measured against that yet) and says so in the log."""
    seg = os.path.join(ROOT, "tests", "golden", "seg", "twopopssplit_unidirmigr_first2Mb.seg")
    L = 2000000
    core = ("-N0 10000 -t %g -r %g %d -I 2 4 4 -eN 0.0 1.0 -ema 0.0 0 0.2 0.2 0 -eN 0.1 1.0 -ema 0.1 0 0.2 0.2 0 "
            "-eN 0.5 1.0 -ema 0.5 0 0 0 0 -ej 0.5 2 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", "8", "-EM", "0", "-tmax", "4", "-seg", seg, "-Np", "1000", "-lag", "50000", "-seed", "5", "-log"]

    def run(name, extra):
        r = subprocess.run([built_binary] + core + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-400:])
        return open(tmp_path / (name + ".out")).read(), r.stderr, open(tmp_path / (name + ".log")).read()

    one, err1, log1 = run("r1", ["-chunks", "3", "-ranks", "1"])
    three, err3, log3 = run("r3", ["-chunks", "3", "-ranks", "3", "-reduce", "host"])
    for log, err in ((log1, err1), (log3, err3)):
        assert log.count("1 chunk(s) ran one after the other") == 3 and err.count("1 chunk(s) ran one after the other") == 3
        assert "side by side" not in log
    assert one == three and "Migr" in one
    for c in range(3):
        rows = []
        for name in ("r1", "r3"):
            lines = gzip.open(tmp_path / ("%s.chunk%d.recomb.gz" % (name, c)), "rt").read().splitlines()
            rows.append([ln.split() for ln in lines[1:]])
        assert len(rows[0]) == len(rows[1]) > 0
        assert [r_[:3] for r_ in rows[0]] == [r_[:3] for r_ in rows[1]]                  # iteration, locus, size
        x = np.array([[float(v) for v in r_[3:]] for r_ in rows[0]]); y = np.array([[float(v) for v in r_[3:]] for r_ in rows[1]])
        assert x.sum() > 0
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-12)          # (five significant digits in the file; sums of atomics)
