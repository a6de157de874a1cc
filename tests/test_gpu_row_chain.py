"""What the shortened row chain of the one-population sweep kernels adds to the existing parity tests.

(i)  The parent search of a resampling row on the path that stages the pilot scans itself: with PF_DEBUG_NO_SPEC_STAGE the
     window requested with the prologue never covers the range of parents, so every resampling row goes through the search
     over the wavefront maxima, the staging round trip and the search inside the wavefront.  Particle counts that are neither a
     multiple of 64 nor of 256 leave a partly filled last wavefront and a partly filled last workgroup (the padding of the
     tables takes part in the searches).
(ii) The row's own segment data is requested with the first loads of a launch and the update loop may not run at all: rows
     whose samples are all missing, rows that end past the sequence length, and both at once.

Everything is compared with the oracle bit for bit: trace, resampling parents, final particles."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

NO_SPEC_STAGE = 32          # PF_DEBUG_NO_SPEC_STAGE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _against_oracle(oracle, model, segs, Np, seed, min_resampling=1, **gpu_kw):
    from smcsmc_amd import ParticleFilter
    o = oracle.Oracle(model, Np, seed=seed, max_trace_events=64)
    o.init_prior(segs["start"][0])
    si = o.pack_segments(model, segs)
    o.run(si)
    g = ParticleFilter(model, Np, seed=seed, max_trace_events=64, **gpu_kw)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    g.run(); g.finish()
    to, tg = o.trace(), g.trace()
    assert g.segments_done() == len(to["T"])
    assert (to["resampled"] == tg["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    so, po = o.resample_events(); sg, pg = g.resample_events()
    assert len(so) >= min_resampling, "the case does not resample: it checks nothing of the parent search"
    assert (so == sg).all() and (po == pg).all()
    ps_o, ps_g = o.particles(), g.particles()
    assert (ps_o["children"] == ps_g["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(ps_o[k]) == _bits(ps_g[k])).all(), k
    assert _bits([o.logl()])[0] == _bits([g.logl()])[0]
    g.close(); o.close()
    return to


@pytest.mark.parametrize("n,Np", [(2, 1000), (3, 1100), (4, 1000), (4, 2500)])
def test_parent_search_outside_the_staged_window(oracle, hiplib, n, Np):
    assert Np % 64 != 0 and Np % 256 != 0
    model = cases.make_model(n=n, E=10, L=1.5e5)
    segs = cases.make_segments(model, seed=20 + n, max_seg_len=4000)
    _against_oracle(oracle, model, segs, Np, seed=9, min_resampling=3, debug=NO_SPEC_STAGE, local_recomb=True)


@pytest.mark.parametrize("n,Np", [(4, 1000), (3, 300)])
def test_rows_without_data_and_rows_past_the_end(oracle, hiplib, n, Np):
    L = 1.2e5
    model = cases.make_model(n=n, E=10, L=L)
    # a block in which every sample is missing (leaf status -1: no mutation weight, no site likelihood) and a block in which
    # some are (the tracked length is recomputed after every update)
    segs = cases.make_segments(model, seed=31, max_seg_len=3000, missing_block=(3.0e4, 5.0e4, list(range(n))))
    al = segs["alleles"]
    part = (segs["start"] >= 7.0e4) & (segs["start"] < 8.0e4)
    al[part, 0] = -1
    rows_all_missing = int((al == -1).all(axis=1).sum())
    assert rows_all_missing >= 3
    # the last row ends past the sequence length, and it carries no data either
    segs["length"][-1] += 7000.0
    al[-1, :] = -1
    assert segs["start"][-1] + segs["length"][-1] > L
    to = _against_oracle(oracle, model, segs, Np, seed=4, local_recomb=True)
    assert len(to["T"]) == len(segs["start"])

    # the same rows on the staging path of (i), and a sequence that ends inside an earlier row: the rows behind it are not run
    _against_oracle(oracle, model, segs, Np, seed=4, debug=NO_SPEC_STAGE)
    short = dict(model, loci_length=9.05e4)
    o_rows = _against_oracle(oracle, short, segs, Np, seed=4, min_resampling=0)
    assert len(o_rows["T"]) < len(segs["start"])
