"""The model flags dephase and ancestral_aware (pf_model.flags bits 1 and 0) on every copy of the site weight's mean over phasings and on
every pruning routine that holds the root prior: the device against the CPU oracle, bit for bit.

Same bar as test_gpu_structured.py / test_gpu_wide_pops.py: trees, node populations and migration lists where there are any, w_post,
w_pilot, next_base, the T, ess and logl columns of the trace, resampling flags and indices bit-identical; count sums within COUNT_RTOL = 1e-9.
The cases are tests/emission_cases.py, which asserts what their data contain; every case asserts run_path() (and row_form() on SweepSplit),
so that it names the copy it ran:

  copy  where                                        case            kernel
  1     pf_hip.hip row_site_lik (mask form)          4-single        k_sweep4
                                                     7-sweep         k_sweep       (odd n: sample 6 has no partner)
                                                     7-no-fuse       k_extend_reg
  2     pf_pair.h, the weight wavefront              4-paired        k_sweep4p
  3     pf_lds_body.h                                9-general       k_extend
                                                     33-wide         k_extend_wide (sample 32 alone in the second mask word)
  4     pf_lds_pipe.h                                9-lockstep      k_sweep_xl    (two chunks through run_many)
  5     pf_mp.hip, LDS form                          9-2-general     k_extend_mp
                                                     5-5-wide-walk   k_extend_mp, eight lineage counters
                                                     6-2-ancient     k_extend_mp, the PF_ANC instance
  6     pf_mp.hip, mask form                         4-2-no-fuse     k_extend_mpr
                                                     6-3-rows        k_sweep_xmp
  7     pf_mp_pipe.h                                 9-2-rows        k_sweep_xlmp

each under dephase, ancestral_aware and both.  The oracle's run of a (shape, flags) pair is computed once and shared by the cases of that
shape.  Every case also asserts that the flag mattered: the oracle's log-likelihood differs from the one without it.

Then the look-ahead under dephase (the reference's "dephase ... (but use phasing for -apf)": the tables are those of the rows as phased,
the site weight is dephased) on k_sweep<..., LOOK> and on the general kernels, and an identity that needs no oracle: dephase on phased rows
equals, bit for bit, no flag on the same rows with every heterozygous pair rewritten as (2, 2)."""
import numpy as np
import pytest

import emission_cases as ec
from test_gpu_wide_pops import COUNT_RTOL, _assert_counts_close, _assert_state_equal, _assert_trace_equal, _bits

pytestmark = pytest.mark.gpu
COUNT_KEYS = ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight")


def _compare(ref, g, P):
    assert ref["trace"]["resampled"].sum() > 0, "the case must exercise resampling"
    assert _bits([g.logl()])[0] == _bits([ref["logl"]])[0]
    _assert_trace_equal(ref, g)
    co, cg = ref["counts"], g.counts()
    if P > 1:
        _assert_state_equal(ref, g)
        _assert_counts_close(co, cg)
    else:
        po, pg = ref["particles"], g.particles()
        assert (po["children"] == pg["children"]).all()
        for k in ("heights", "w_post", "w_pilot", "next_base"):
            assert (_bits(po[k]) == _bits(pg[k])).all(), k
        for k in COUNT_KEYS:
            np.testing.assert_allclose(cg[k], co[k], rtol=COUNT_RTOL, atol=1e-300, err_msg=k)
        assert cg["resample_count"] == co["resample_count"]


def _flag_mattered(shape, flags, lookahead=0):
    plain = ec.oracle_run(shape, None, lookahead)["logl"]
    mine = ec.oracle_run(shape, flags, lookahead)["logl"]
    assert mine != plain, "%s: the oracle's log-likelihood under %s is the one without" % (shape, flags)
    if flags == "both":
        assert mine != ec.oracle_run(shape, "dephase", lookahead)["logl"] and mine != ec.oracle_run(shape, "ancestral_aware", lookahead)["logl"]


def _new(shape, flags, seed=None, segs=None, **kw):
    from smcsmc_amd import ParticleFilter
    s = ec.SHAPES[shape]
    segs = ec.rows(shape)[1] if segs is None else segs
    g = ParticleFilter(ec.model(shape, flags), s["Np"], ess_fraction=0.5, seed=s["seed"] if seed is None else seed, max_trace_events=64, **kw)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    return g


@pytest.mark.parametrize("flags", list(ec.FLAGS))
@pytest.mark.parametrize("case_id", ec.IDS)
def test_flagged_sweep_parity(hiplib, oracle, case_id, flags):
    from smcsmc_amd import ParticleFilter
    c = ec.by_id(case_id)
    shape = c["shape"]
    P = ec.SHAPES[shape]["P"]
    _flag_mattered(shape, flags)
    ref = ec.oracle_run(shape, flags)
    fs = [_new(shape, flags, **c["kw"])]
    try:
        if c["how"] == "many":
            # a second chunk beside it: the same rows under another seed
            fs.append(_new(shape, flags, seed=ec.SHAPES[shape]["seed"] + 1, **c["kw"]))
            assert ParticleFilter.can_run_many(fs) and all(f.run_path(many=True) == c["path"] for f in fs)
            ParticleFilter.run_many(fs)
        else:
            assert fs[0].run_path() == c["path"]
            fs[0].run()
        for f in fs:
            f.finish()
        if c["path"] == "SweepSplit":
            assert fs[0].row_form() == c["form"]
        _compare(ref, fs[0], P)
        if len(fs) > 1:
            assert fs[1].segments_done() == fs[0].segments_done() and np.isfinite(fs[1].logl()) and fs[1].logl() != fs[0].logl()
    finally:
        for f in fs:
            f.close()


@pytest.mark.parametrize("pipeline,path", [(True, "Sweep"), (False, "General")], ids=["rows", "general"])
def test_look_ahead_uses_the_phasing_and_the_site_weight_does_not(hiplib, oracle, pipeline, path):
    """n = 8, dephase, -apf 2: k_sweep<..., LOOK> and the general kernels against the oracle.  The look-ahead moves the pilot weights, and
    dephase moves the result with the look-ahead on."""
    shape = "8-apf"
    la, tbl = ec.lookahead_inputs(shape)
    _flag_mattered(shape, "dephase", ec.APF_LEVEL)
    ref = ec.oracle_run(shape, "dephase", ec.APF_LEVEL)
    assert ref["logl"] != ec.oracle_run(shape, "dephase", 0)["logl"]
    g = _new(shape, "dephase")
    try:
        g.load_lookahead(la, ec.APF_LEVEL, tbl, pipeline=pipeline)
        assert g.run_path() == path
        g.run(); g.finish()
        _compare(ref, g, 1)
        pg = g.particles()
        assert (pg["w_post"] != pg["w_pilot"]).any()
    finally:
        g.close()


@pytest.mark.parametrize("shape,kw,path,form", [("4", dict(), "SweepSplit", "paired"), ("9", dict(), "General", None)], ids=["4-paired", "9-general"])
def test_dephase_on_phased_rows_is_no_flag_on_marked_rows(hiplib, shape, kw, path, form):
    """With dephase a phased heterozygous pair is treated exactly as a marked one: same first phasing (0, 1), same order of summation.  So the
    two runs agree in every bit, on one mask-form copy and one LDS copy -- whatever the oracle says.  It fails if a copy starts the
    enumeration at the data's phase, or reads the flag from another bit."""
    phased, marked = ec.identity_rows(shape)
    a = _new(shape, "dephase", segs=phased, **kw)
    b = _new(shape, None, segs=marked, **kw)
    c = _new(shape, None, segs=phased, **kw)
    try:
        for f in (a, b, c):
            assert f.run_path() == path
            f.run(); f.finish()
            if form:
                assert f.row_form() == form
        assert a.logl() != c.logl(), "dephase must move the result on these rows"
        assert a.trace()["resampled"].sum() > 0
        assert _bits([a.logl()])[0] == _bits([b.logl()])[0]
        ta, tb = a.trace(), b.trace()
        assert (ta["resampled"] == tb["resampled"]).all()
        for k in ("T", "ess", "logl"):
            assert (_bits(ta[k]) == _bits(tb[k])).all(), k
        sa, pa = a.resample_events(); sb, pb = b.resample_events()
        assert (sa == sb).all() and (pa == pb).all()
        wa, wb = a.particles(), b.particles()
        assert (wa["children"] == wb["children"]).all()
        for k in ("heights", "w_post", "w_pilot", "next_base"):
            assert (_bits(wa[k]) == _bits(wb[k])).all(), k
        ca, cb = a.counts(), b.counts()
        for k in COUNT_KEYS:                                   # (the lagged sums by the project's bound for them, as against the oracle)
            np.testing.assert_allclose(ca[k], cb[k], rtol=COUNT_RTOL, atol=1e-300, err_msg=k)
        assert ca["resample_count"] == cb["resample_count"]
    finally:
        for f in (a, b, c):
            f.close()


@pytest.mark.parametrize("pair", [(-1, 2), (2, 0), (1, 2)], ids=["missing-mark", "mark-zero", "one-mark"])
def test_a_lone_mark_is_refused(hiplib, pair):
    """pf_load_segments refuses a row in which one sample only of a pair carries the unphased mark, in the words of the .seg readers; the
    mask forms and the LDS forms of the phasing test would disagree on (-1, 2) under dephase.  The handle then still loads a valid set and runs."""
    from smcsmc_amd import ParticleFilter, PfError
    import cases
    m = dict(cases.make_model(n=4, E=4, L=4.0e4), dephase=True)
    good = cases.make_segments(m, seed=3, unphased=True, max_seg_len=5000)
    al = np.array(good["alleles"], np.int8).reshape(len(good["start"]), 4)
    site = int(np.nonzero(np.asarray(good["state"]) == 0)[0][1])
    al[site, 2:4] = pair
    g = ParticleFilter(m, 128, seed=2)
    try:
        g.init_prior(good["start"][0])
        with pytest.raises(PfError, match="Found inconsistent unphased heterozygous marks"):
            g.load_segments(dict(good, alleles=al))
        al[site, 2:4] = (0, 3)
        with pytest.raises(PfError, match="Unknown character"):
            g.load_segments(dict(good, alleles=al))
        g.load_segments(good)
        g.run(); g.finish()
        assert g.segments_done() == len(good["start"]) and np.isfinite(g.logl())
    finally:
        g.close()
