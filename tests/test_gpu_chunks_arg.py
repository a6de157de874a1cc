"""Tree dumps and resampling positions per chunk (bin/smcsmc -arg -record_ess -chunks K -ranks R), and what the binary rests
on: tree recording in lockstep (pf_run_many with record_trees, the TREES instances of k_sweep / k_sweep4) gives every chunk the
dump of its own run().  The reference's front-end passes -arg to every chunk process (smcsmc/model.py:1062-1063, 1094-1098); here
every chunk of one process leaves <prefix>.chunkN.trees.gz and <prefix>.chunkN.resample, whichever way the chunks are spread over
ranks and whether or not a group shared its launches."""
import functools
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import trees_format
from smcsmc_amd import ParticleFilter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "smcsmc")
SEG = os.path.join(ROOT, "tests", "golden", "seg", "constpopsize.seg")
L = 4000000
HALF = L // 2
# CORE / COMMON of tests/test_gpu_chunks.py
CORE = ("-N0 10000 -t %g -r %g %d -eN 0 1 -eN 0.01 1 -eN 0.25 1 -eN 1 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
COMMON = ["-nsam", "2", "-seg", SEG, "-Np", "300", "-tmax", "4", "-lag", "30000", "-seed", "5"]
ESS = ["-ESS", "0.7"]
ARG = ["-arg", "-record_ess"] + ESS + ["-chunks", "2"]


def _binary(tmp, name, args):
    r = subprocess.run([BIN] + args + ["-o", os.path.join(tmp, name)], capture_output=True, text=True)
    assert r.returncode == 0, (name, (r.stderr + r.stdout)[-600:])
    return r.stderr


def _bytes(tmp, name, suffix):
    with open(os.path.join(tmp, name + suffix), "rb") as f:
        return f.read()


def _tree_lines(tmp, name, c):
    return gzip.open(os.path.join(tmp, "%s.chunk%d.trees.gz" % (name, c)), "rt").read().splitlines()


def _resample_rows(tmp, name, c):
    return [(int(a), float(b)) for a, b in (ln.split("\t") for ln in open(os.path.join(tmp, "%s.chunk%d.resample" % (name, c))).read().splitlines())]


@pytest.fixture(scope="module")
def lockstep_run(hiplib, tmp_path_factory):
    """Test 1's run, made once and only read afterwards: two chunks of one rank, with -arg -record_ess."""
    tmp = str(tmp_path_factory.mktemp("chunks_arg"))
    log = _binary(tmp, "ls", CORE + COMMON + ARG + ["-ranks", "1"])
    return tmp, log


def test_two_chunks_in_lockstep_leave_their_tree_dumps(lockstep_run):
    tmp, log = lockstep_run
    assert "chunks 0 to 1: 2 chunk(s) ran side by side" in log
    note = open(os.path.join(tmp, "ls.log")).read()
    assert "2 chunk(s) ran side by side" in note
    assert not os.path.exists(os.path.join(tmp, "ls.trees.gz")) and not os.path.exists(os.path.join(tmp, "ls.resample"))
    for c in range(2):
        assert os.path.exists(os.path.join(tmp, "ls.chunk%d.trees.gz" % c)) and os.path.exists(os.path.join(tmp, "ls.chunk%d.recomb.gz" % c))
        assert "chunk %d: trees written to %s" % (c, os.path.join(tmp, "ls.chunk%d.trees.gz" % c)) in note
        lines = _tree_lines(tmp, "ls", c)
        trees_format.check_lines(lines, nsam=2, npop=1)
        fields = [ln.split("\t") for ln in lines]
        assert len(lines) > 10 and {f[0] for f in fields} == {"R", "C"}
        # positions are those of the whole sequence: the writer adds the chunk's first base
        pos = np.array([float(f[1]) for f in fields])
        assert pos.min() >= c * HALF and pos.max() <= (c + 1) * HALF, (c, pos.min(), pos.max())
        assert fields[-1][0] == "C" and fields[-1][5] == "11" and float(fields[-1][1]) == c * HALF    # the first tree: sample 2 joins sample 1
        # .resample: the end of every row that was followed by a resampling, counted from the chunk's first base as the reference's
        # chunk process counts them (update_to, particleContainer.cpp:288), and the ESS there
        rows = _resample_rows(tmp, "ls", c)
        assert len(rows) >= 1
        assert all(0 < p <= HALF and 0.0 < e <= 300.0 for p, e in rows), rows[:5]
        assert all(b[0] > a[0] for a, b in zip(rows, rows[1:]))
    # tree recording changes no statistic.  Without -arg two haplotypes run as two launches a step (SweepSplit), with it as one (Sweep):
    # the ledger and count roles are the same code with the same workgroups in either, so the sums are grouped alike -- byte for byte
    _binary(tmp, "plain", CORE + COMMON + ESS + ["-chunks", "2", "-ranks", "1"])
    assert _bytes(tmp, "ls", ".out") == _bytes(tmp, "plain", ".out")


def test_files_of_a_chunk_do_not_depend_on_the_ranks(lockstep_run):
    """Two ranks, one chunk each: every chunk goes through pf_run alone.  Its four files are those of the lockstep run, byte for
    byte -- lockstep equals alone, at the level of the files."""
    tmp, _ = lockstep_run
    log = _binary(tmp, "r2", CORE + COMMON + ARG + ["-ranks", "2", "-reduce", "host"])
    assert "2 rank(s)" in log and "side by side" not in log
    for c in range(2):
        for suffix in (".chunk%d.trees.gz" % c, ".chunk%d.resample" % c):
            assert _bytes(tmp, "r2", suffix) == _bytes(tmp, "ls", suffix), suffix
    assert _bytes(tmp, "r2", ".out") == _bytes(tmp, "ls", ".out")


def test_every_e_step_overwrites_the_trees_and_appends_resample_rows(lockstep_run):
    tmp, _ = lockstep_run
    _binary(tmp, "em", CORE + COMMON + ARG + ["-ranks", "1", "-EM", "1"])
    for c in range(2):
        # one dump, that of the last iteration: the grammar of a single dump (positions never rise again: check_lines), ending in the
        # first tree; and not the dump of iteration 0, which the lockstep run left
        lines = _tree_lines(tmp, "em", c)
        trees_format.check_lines(lines, nsam=2, npop=1)
        assert len(lines) > 10
        assert [ln for ln in lines if float(ln.split("\t")[1]) == c * HALF and ln[0] == "C"] == [lines[-1]]
        assert lines != _tree_lines(tmp, "ls", c)
        # rows of both iterations: iteration 0 is the lockstep run's file (same seed, same model), iteration 1 follows it
        first = _resample_rows(tmp, "ls", c)
        both = _resample_rows(tmp, "em", c)
        assert both[:len(first)] == first and len(both) > len(first)
        assert sum(1 for a, b in zip(both, both[1:]) if b[0] <= a[0]) == 1
    iters = {ln.split()[0] for ln in open(os.path.join(tmp, "em.out")).read().splitlines()[1:]}
    assert iters == {"0", "1"}


def test_chunk_one_is_the_library_run_of_its_window(lockstep_run):
    """Chunk 1 through the python binding, as test_gpu_parity.py::test_binary_writes_the_tree_dump reproduces a whole window: the rows
    of [first[1], first[1] + 2 000 000), the binary's per-base rates, seed 5 + 1 (seed + 1000 * iteration + chunk)."""
    from smcsmc_amd import outfile, segments as segmod
    tmp, _ = lockstep_run
    m = json.loads(subprocess.run([BIN] + CORE + ["-nsam", "2", "-tmax", "4", "-dumpmodel"], capture_output=True, text=True).stdout)
    E = len(m["change_times"])
    model = dict(change_times=np.array(m["change_times"]), pop_sizes=np.array(m["pop_sizes"])[:, 0], lags=np.full(E, 30000.0),
                 nsam=2, loci_length=float(HALF), mutation_rate=m["mutation_rate"], recombination_rate=m["recombination_rate"])
    first1 = 1 + HALF
    S = segmod.Segments(SEG, 2, HALF, data_start=first1, max_segment_length=int(2.0 / (m["recombination_rate"] * 4 * m["N0"])))
    segs = S.pack(model["lags"])
    rows = len(segs["start"])
    log_cap = 16384
    while log_cap < 1.4 * rows:
        log_cap *= 2
    gen_cap = 16384
    while gen_cap < rows + 2:
        gen_cap *= 2
    g = ParticleFilter(model, 300, ess_fraction=0.7, seed=5 + 1, max_trace_events=0, local_recomb=True, record_trees=True,
                       log_cap=log_cap, gen_cap=gen_cap)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    _, kind, pos, hgt, desc = g.sample_tree_events()
    g.close()
    text = gzip.open(os.path.join(tmp, "ls.chunk1.trees.gz"), "rt").read()
    assert outfile.trees_text(kind, pos, hgt, desc, start_position=float(first1)) == text


def test_chunks_of_a_structured_model_leave_their_tree_dumps(hiplib, tmp_path):
    """Two populations, four haplotypes: -arg runs on the general kernels, which pf_run_many refuses -- the chunks are filtered one
    after the other, and their dumps carry the M lines; the same files from two ranks."""
    from smcsmc_amd import simulate
    tmp = str(tmp_path)
    n, Ls = 4, 200000
    base = cases.make_model(n=n, E=8, L=float(Ls))
    seg = os.path.join(tmp, "d.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, float(Ls), base["mutation_rate"], base["recombination_rate"], base["change_times"],
                                                  base["pop_sizes"], seed=44))
    core = ("-N0 10000 -t %g -r %g %d -I 2 2 2 -eN 0.0 1.0 -ema 0.0 0 2.0 2.0 0 -eN 0.1 1.0 -ema 0.1 0 2.0 2.0 0 "
            "-eN 0.5 1.0 -ema 0.5 0 0 0 0 -ej 0.5 2 1" % (4e4 * 2.5e-8 * Ls, 4e4 * 1e-8 * Ls, Ls)).split()
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg, "-Np", "160", "-seed", "5", "-lag", "50000", "-arg", "-chunks", "2"]
    log = _binary(tmp, "s1", core + common + ["-ranks", "1"])
    assert "one after the other" in log and "side by side" not in log
    _binary(tmp, "s2", core + common + ["-ranks", "2", "-reduce", "host"])
    codes = set()
    for c in range(2):
        lines = _tree_lines(tmp, "s1", c)
        trees_format.check_lines(lines, nsam=n, npop=2)
        fields = [ln.split("\t") for ln in lines]
        assert len(lines) > 10 and "R" in {f[0] for f in fields}
        pos = np.array([float(f[1]) for f in fields])
        assert pos.min() >= c * (Ls // 2) and pos.max() <= (c + 1) * (Ls // 2)
        codes |= {f[0] for f in fields}
        assert _bytes(tmp, "s2", ".chunk%d.trees.gz" % c) == _bytes(tmp, "s1", ".chunk%d.trees.gz" % c)
    assert codes == {"R", "C", "M"}
    assert not os.path.exists(os.path.join(tmp, "s1.trees.gz"))


# ---------------------------------------------------------------- the library: tree recording in lockstep

NP = 200             # not a multiple of 64
E_LIB = 8
ESS_LIB = 0.9        # most rows resample
# two chunks of every shape: lengths (different numbers of rows), seeds, and ring capacities that differ between the chunks
CHUNKS = ((2.4e5, 21, dict(log_cap=8192, gen_cap=2048)), (0.8e5, 22, dict(log_cap=4096, gen_cap=1024)))
CALL = 100           # rows per run_many call: the short chunk sits the last calls out
SHAPES = [(2, "plain"), (4, "plain"), (5, "plain"), (8, "plain"), (4, "focused"), (8, "guide")]


@functools.lru_cache(maxsize=None)
def _chunk_inputs(n, kind, k):
    length, seed, _ = CHUNKS[k]
    model = cases.make_model(n=n, E=E_LIB, L=length)
    segs = cases.make_segments(model, seed=seed + n, max_seg_len=4000)
    if kind == "focused":
        model = dict(model, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(E_LIB, 3000.0), delay_type=0)
    elif kind == "guide":
        model = dict(model, guide=cases.guide(model, 5, 2.5, n), application_delays=np.full(E_LIB, 3000.0))
    return model, segs


def _recording_filter(n, kind, k):
    model, segs = _chunk_inputs(n, kind, k)
    f = ParticleFilter(model, NP, ess_fraction=ESS_LIB, seed=7 + k, max_trace_events=0, record_trees=True, **CHUNKS[k][2])
    f.init_prior(segs["start"][0]); f.load_segments(segs)
    return f


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("n,kind", SHAPES, ids=["n%d-%s" % s for s in SHAPES])
def test_lockstep_tree_recording_equals_each_filter_alone(hiplib, n, kind):
    """Two tree-recording chunks through pf_run_many, then finish(): the one-particle draw and the events of its history, the
    likelihood, the resampling trace and the counts are those of the same chunks run alone -- the dump bit for bit, the counts as
    tests/test_gpu_sweep.py compares lockstep with alone (bit for bit: same workgroups, same order)."""
    many = [_recording_filter(n, kind, k) for k in range(2)]
    alone = [_recording_filter(n, kind, k) for k in range(2)]
    try:
        assert all(f.run_path(many=True) == "Sweep" for f in many)           # (it cannot pass by falling back)
        assert ParticleFilter.can_run_many(many)
        nmax = max(f.n_segs for f in many)
        assert 200 <= nmax < 1000 and many[1].n_segs <= CALL * ((nmax - 1) // CALL)      # a few hundred rows; chunk 1 sits at least the last call out
        for s0 in range(0, nmax, CALL):
            ParticleFilter.run_many(many, s0, min(nmax, s0 + CALL))
        for f in many:
            f.finish()
        for g in alone:
            g.run(); g.finish()
        for k, (f, g) in enumerate(zip(many, alone)):
            assert f.segments_done() == g.segments_done() == f.n_segs
            pf_, kf, xf, hf, df = f.sample_tree_events(pops=False)
            pg, kg, xg, hg, dg = g.sample_tree_events(pops=False)
            assert len(kg) > 10 and (kg == 0).any(), "chunk %d: the case must record recombinations" % k
            assert pf_ == pg and len(kf) == len(kg), "chunk %d: particle %d / %d, %d / %d events" % (k, pf_, pg, len(kf), len(kg))
            assert (kf == kg).all() and (df == dg).all()
            assert (_bits(xf) == _bits(xg)).all() and (_bits(hf) == _bits(hg)).all()
            assert _bits(f.logl()) == _bits(g.logl())
            rf, rg = f.trace()["resampled"], g.trace()["resampled"]
            assert (rf == rg).all() and rg.sum() > 0.5 * len(rg)             # most rows resample
            cf, cg = f.counts(), g.counts()
            for key in cg:
                assert (_bits(cf[key]) == _bits(cg[key])).all(), key
    finally:
        for f in many + alone:
            f.close()


def test_a_recording_handle_does_not_run_with_a_plain_one(hiplib):
    """sweep_compatible compares rec_trees: eight haplotypes run as k_sweep with and without tree recording, each handle is taken
    on its own, the pair is refused."""
    model, segs = _chunk_inputs(8, "plain", 1)
    a = ParticleFilter(model, NP, seed=7, max_trace_events=0, record_trees=True, log_cap=4096, gen_cap=1024)
    b = ParticleFilter(model, NP, seed=8, max_trace_events=0)
    try:
        for f in (a, b):
            f.init_prior(segs["start"][0]); f.load_segments(segs)
            assert f.run_path(many=True) == "Sweep" and ParticleFilter.can_run_many([f])
        assert not ParticleFilter.can_run_many([a, b])
        assert not ParticleFilter.can_run_many([b, a])
    finally:
        a.close(); b.close()
