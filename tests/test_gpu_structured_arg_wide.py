"""Tree dumps (-arg) of structured models on the LDS-tree row kernel (k_extend_mp<BIASED, TREES>): 9 to 16 haplotypes,
and at most 8 with PF_DEBUG_FORCE_LDS, against the CPU oracle -- the dump of the drawn particle event for event, the
sweep itself (trace, particles, counts) with tree recording on, the step API, the ring-overflow error and the binary.
The cases are those of test_gpu_structured.py::test_tree_dump_with_structure at more haplotypes."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

E = 8
FORCE_LDS = 1
RINGS = dict(record_trees=True, log_cap=8192, gen_cap=4096)
COUNT_COLUMNS = ("coal_count", "coal_opp", "rec_count", "rec_opp", "mig_count", "mig_opp")
DUMP_NAMES = ("kind", "pos", "height", "desc", "from_pop", "to_pop")

# (n, P, Np, split_epoch, focused sampling)
DUMP_CASES = [(9, 2, 160, E - 3, False), (12, 2, 160, E, False), (16, 2, 128, E, False), (12, 3, 160, E - 3, True),
              (16, 4, 128, E - 3, False)]
NO_JOIN_12 = (12, 2, 160, E, False)
JOINED_16 = (16, 4, 128, E - 3, False)
LOCAL_MAP_CASES = {NO_JOIN_12}           # the oracle records the local recombination map for these as well


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _inputs(case):
    n, P, Np, split, bias = case
    base = cases.make_model(n=n, E=E, L=1.2e5)
    segs = cases.make_segments(base, seed=40 + n, max_seg_len=5000)
    model = cases.make_structured(base, P=P, split_epoch=split, mig=2.0)
    if bias:
        model = dict(model, bias_heights=[400.0], bias_strengths=[4.0, 1.0], application_delays=np.full(E, 3000.0))
    return model, segs


_ORACLE = {}


def _oracle_run(oracle, case):
    """The oracle's run of a case with tree recording on, computed once per session and only read afterwards."""
    if case not in _ORACLE:
        model, segs = _inputs(case)
        o = oracle.Oracle(model, case[2], seed=5, max_trace_events=0)
        o.enable_tree_recording()
        if case in LOCAL_MAP_CASES:
            o.enable_local_recomb()
        o.init_prior(segs["start"][0]); o.run(o.pack_segments(model, segs))
        ref = dict(dump=o.sample_tree_events(pops=True), trace=o.trace(), particles=o.particles(), migrations=o.migrations(),
                   counts=o.counts())
        if case in LOCAL_MAP_CASES:
            ref["lmap"] = o.local_recomb(model["loci_length"])
        _ORACLE[case] = ref
    return _ORACLE[case]


def _filter(case, **kw):
    from smcsmc_amd import ParticleFilter
    model, segs = _inputs(case)
    g = ParticleFilter(model, case[2], seed=5, max_trace_events=0, **dict(RINGS, **kw))
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    return g


def _device_run(case, **kw):
    g = _filter(case, **kw)
    g.run(); g.finish()
    return g


def _assert_dumps_equal(a, b):
    assert a[0] == b[0] and len(a[1]) == len(b[1]), "sampled particle %d / %d, %d / %d events" % (a[0], b[0], len(a[1]), len(b[1]))
    for name, x, y in zip(DUMP_NAMES, a[1:], b[1:]):
        if name in ("pos", "height"):
            assert (_bits(x) == _bits(y)).all(), name
        else:
            assert (np.asarray(x) == np.asarray(y)).all(), name


def _walk(dump, n, P):
    """The structure of a dump (test_tree_dump_with_structure): every update reads R, C, then the migrations of its walk.
    Returns the number of M lines and of those on the root's own lineage (descendants = everything but the cut samples)."""
    _, kind, pos, hgt, desc, fr, to = dump
    assert (np.diff(pos) <= 0).all()
    full = (1 << n) - 1
    n_m = n_root = 0
    i = 0
    while i < len(kind):
        if kind[i] == 0:                       # an update: R, C, M...
            cut = int(desc[i]); x = pos[i]; i += 1
            assert kind[i] == 1 and pos[i] == x and hgt[i] >= hgt[i - 1] and (int(desc[i]) & cut) == cut
        else:                                  # a leaf of the first tree: C, M...
            assert kind[i] == 1 and pos[i] == 0.0
            cut = None
        tc = hgt[i]; i += 1
        while i < len(kind) and kind[i] == 2:
            assert hgt[i] <= tc and fr[i] != to[i] and 0 <= to[i] < P
            n_m += 1
            if cut is not None:
                assert int(desc[i]) in (cut, full & ~cut)
                n_root += int(desc[i]) == (full & ~cut)
            i += 1
    return n_m, n_root


def _canon_events(mg):
    out = []
    for i in range(len(mg["n_events"])):
        k = mg["n_events"][i]
        out.append(sorted(zip(_bits(mg["times"][i, :k]).tolist(), mg["branch"][i, :k].tolist(), mg["newpop"][i, :k].tolist())))
    return out


@pytest.mark.parametrize("case", DUMP_CASES, ids=lambda c: "n%d-P%d-split%d%s" % (c[0], c[1], c[3], "-focused" if c[4] else ""))
def test_wide_structured_dump_equals_the_oracle(oracle, hiplib, case):
    """The R, C and M lines of the drawn particle's history at 9 to 16 haplotypes: sampled particle, kinds, descendant sets
    and populations equal, positions and heights bit for bit."""
    from smcsmc_amd import outfile
    n, P, Np, split, bias = case
    ref = _oracle_run(oracle, case)
    g = _device_run(case)
    dump = g.sample_tree_events(pops=True)
    _assert_dumps_equal(ref["dump"], dump)
    # the case cannot pass empty
    assert g.trace()["resampled"].sum() > 3
    n_m, n_root = _walk(dump, n, P)
    assert n_m >= 1, "the case must exercise migrations"
    assert (np.asarray(dump[4]) >> 8).any(), "no descendant set reaches sample 8 or beyond"
    if split == E:
        assert n_root >= 1, "a model without a join must put migrations on the root's own lineage"
    _, kind, pos, hgt, desc, fr, to = dump
    text = outfile.trees_text(kind, pos, hgt, desc, start_position=1.0, from_pop=fr, to_pop=to)
    assert len(text.splitlines()) == len(kind) and any(ln.startswith("M\t") for ln in text.splitlines())


@pytest.mark.parametrize("case", [NO_JOIN_12, JOINED_16], ids=["n12-P2-nojoin-localmap", "n16-P4"])
def test_sweep_is_unchanged_by_tree_recording(oracle, hiplib, case):
    """With -arg on, the meta word of a record holds a descendant set where it otherwise holds the epoch span of its pieces:
    trace and final particles still equal the oracle's bit for bit, the counts (and the local map, where recorded) within
    the tolerance of every structured parity test."""
    ref = _oracle_run(oracle, case)
    lmap = case in LOCAL_MAP_CASES
    g = _device_run(case, local_recomb=lmap)
    to, tg = ref["trace"], g.trace()
    assert g.segments_done() == len(to["T"])
    assert (to["resampled"] == tg["resampled"]).all() and to["resampled"].sum() > 3
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    po, pg = ref["particles"], g.particles()
    assert (po["children"] == pg["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(po[k]) == _bits(pg[k])).all(), k
    mo, mg = ref["migrations"], g.migrations()
    assert (mo["n_events"] == mg["n_events"]).all() and (mo["node_pops"] == mg["node_pops"]).all()
    assert _canon_events(mo) == _canon_events(mg)
    co, cg = ref["counts"], g.counts()
    assert co["mig_count"].sum() > 0
    for k in COUNT_COLUMNS:
        print(k, "largest difference", np.abs(cg[k] - co[k]).max(), "column scale", np.abs(co[k]).max())
        np.testing.assert_allclose(cg[k], co[k], rtol=1e-9, atol=1e-9 * np.abs(co[k]).max(), err_msg=k)
    if lmap:
        lo, lg = ref["lmap"], g.local_recomb()
        cso, csg = np.cumsum(lo["opp_diff"]), np.cumsum(lg["opp_diff"])      # the differential form cancels large terms
        assert cso.max() > 0 and lo["counts"][:case[0]].sum() > 0
        np.testing.assert_allclose(csg, cso, rtol=1e-7, atol=1e-7 * cso.max())
        np.testing.assert_allclose(lg["counts"], lo["counts"], rtol=1e-9, atol=1e-12 * max(1.0, lo["counts"].max()))


@pytest.mark.parametrize("case", [(8, 2, 160, E - 3, False), (6, 3, 200, E - 3, True)], ids=["n8-P2", "n6-P3-focused"])
def test_both_row_kernels_give_the_same_dump(oracle, hiplib, case):
    """At most 8 haplotypes: the register-tree kernel and, with PF_DEBUG_FORCE_LDS, the LDS-tree kernel record the same
    trees, and both are the oracle's."""
    ref = _oracle_run(oracle, case)
    reg = _device_run(case).sample_tree_events(pops=True)
    lds = _device_run(case, debug=FORCE_LDS).sample_tree_events(pops=True)
    _assert_dumps_equal(reg, lds)
    _assert_dumps_equal(ref["dump"], lds)
    _assert_dumps_equal(ref["dump"], reg)
    assert _walk(lds, case[0], case[1])[0] >= 1


def test_step_api_gives_the_dump_of_run(oracle, hiplib):
    case = NO_JOIN_12
    _, segs = _inputs(case)
    a = _device_run(case).sample_tree_events(pops=True)
    g = _filter(case)
    for s in range(len(segs["start"])):
        g.update_segment(s); g.count(s); g.resample(s)
    g.finish()
    b = g.sample_tree_events(pops=True)
    _assert_dumps_equal(a, b)
    _assert_dumps_equal(_oracle_run(oracle, case)["dump"], b)


def test_ring_too_small_for_the_trees_is_a_reported_error(oracle, hiplib):
    """-arg keeps every record: a record ring that cannot hold them stops the run with the library's ring-overflow error
    (the write position wraps inside the ring, nothing else is touched), and the next filter of the process is unaffected."""
    from smcsmc_amd.pf import PfError
    case = NO_JOIN_12
    with pytest.raises(PfError, match="event log ring overflow"):
        g = _filter(case, log_cap=64)
        g.run(); g.finish()
    g.close()
    dump = _device_run(case).sample_tree_events(pops=True)
    _assert_dumps_equal(_oracle_run(oracle, case)["dump"], dump)


def test_binary_writes_a_structured_tree_dump_of_twelve_haplotypes(hiplib, tmp_path):
    """bin/smcsmc -arg on two populations of six haplotypes each: the .trees.gz follows the grammar of the reference's
    example file, names samples beyond the eighth, and equals line for line what the python binding writes for the same
    run; more than 16 haplotypes with structure stay refused."""
    import gzip
    import json
    import os
    import subprocess
    import trees_format
    from smcsmc_amd import ParticleFilter, outfile, simulate, segments as segmod
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "bin", "smcsmc")
    n, L = 12, 120000
    base = cases.make_model(n=n, E=E, L=float(L))
    seg = str(tmp_path / "d.seg")
    simulate.write_seg(seg, simulate.simulate_seg(n, float(L), base["mutation_rate"], base["recombination_rate"], base["change_times"],
                                                  base["pop_sizes"], seed=40 + n))
    core = ("-N0 10000 -t %g -r %g %d -I 2 6 6 -eN 0.0 1.0 -ema 0.0 0 2.0 2.0 0 -eN 0.1 1.0 -ema 0.1 0 2.0 2.0 0 "
            "-eN 0.5 1.0 -ema 0.5 0 0 0 0 -ej 0.5 2 1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    common = ["-nsam", str(n), "-EM", "0", "-tmax", "4", "-seg", seg]
    r = subprocess.run([binary] + core + common + ["-Np", "160", "-seed", "5", "-lag", "50000", "-arg", "-o", str(tmp_path / "arg")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = gzip.open(tmp_path / "arg.trees.gz", "rt").read()
    raw_lines = text.splitlines()
    trees_format.check_lines(raw_lines, nsam=n, npop=2)
    fields = [ln.split("\t") for ln in raw_lines]
    assert {f[0] for f in fields} == {"R", "C", "M"}
    assert any(len(f[5]) > 8 for f in fields), "no descendant list names a sample index >= 8"
    m = json.loads(subprocess.run([binary] + core + ["-nsam", str(n), "-tmax", "4", "-dumpmodel"], capture_output=True, text=True).stdout)
    Em = len(m["change_times"])
    assert m["npop"] == 2 and m["sample_pops"] == [0] * 6 + [1] * 6
    mig = np.array(m["mig_rates"]).reshape(Em, 2, 2); smig = np.array(m["single_mig"]).reshape(Em, 2, 2)
    model = dict(change_times=np.array(m["change_times"]), pop_sizes=np.array(m["pop_sizes"]), lags=np.full(Em, 50000.0),
                 nsam=n, loci_length=float(L), mutation_rate=m["mutation_rate"], recombination_rate=m["recombination_rate"],
                 n_pops=2, mig_rates=mig, single_mig=smig, sample_pops=m["sample_pops"])
    S = segmod.Segments(seg, n, L, max_segment_length=int(2.0 / (m["recombination_rate"] * 4 * m["N0"])))
    segs = S.pack(model["lags"])
    g = ParticleFilter(model, 160, seed=5, max_trace_events=0, local_recomb=True, record_trees=True, log_cap=16384, gen_cap=8192)
    g.init_prior(segs["start"][0]); g.load_segments(segs); g.run(); g.finish()
    _, kind, pos, hgt, desc, fr, to = g.sample_tree_events(pops=True)
    assert outfile.trees_text(kind, pos, hgt, desc, start_position=1.0, from_pop=fr, to_pop=to) == text
    # structured models stop at 16 haplotypes, with or without -arg
    i = core.index("-I")
    core18 = core[:i + 2] + ["9", "9"] + core[i + 4:]
    r = subprocess.run([binary] + core18 + ["-nsam", "18", "-EM", "0", "-tmax", "4", "-seg", seg, "-Np", "160", "-arg", "-o", str(tmp_path / "no")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "more than 16 haplotypes need one population" in r.stderr + r.stdout
