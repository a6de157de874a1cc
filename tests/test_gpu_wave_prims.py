"""The wavefront sums and scans without LDS (pf_device.h) against the forms they replace, and two sweeps wide enough for the second
level of decide_row.

(i)  pf_probe_wave_prims runs every primitive in both forms on wavefronts of 64 values from the host: the form that moves operands
     with __shfl_xor / __shfl_up and the form that moves them with DPP and the lane swaps.  4 096 wavefronts in one call; equal
     bits lane by lane.  No NaN (out of scope for both forms: which payload survives an addition depends on the operand order).
(ii) Two sweeps against the oracle, bit for bit, with the comparison of test_gpu_row_chain.py.  Np = 4 200 has 66 wavefront
     partials, so the second level of decide_row has two groups, the second with two entries, and the last wavefront 40 lanes;
     Np = 8 250 has 129 partials, three groups as the headline shape's 157, and a partly filled last wavefront and workgroup.  The
     other tests stop at 2 500 particles: 40 partials, one group.  The oracle takes 4 s and 9 s on these (the model and the counts are
     the smallest that reach the path), so it runs once per count and both sweeps of a count are held to that one run."""
import numpy as np
import pytest

import cases
from test_gpu_row_chain import NO_SPEC_STAGE, _bits

pytestmark = pytest.mark.gpu

K = 4096
I32 = np.iinfo(np.int32)


def _doubles():
    rng = np.random.default_rng(141)
    x = np.empty((K, 64))
    names = {}
    r = 0

    def put(name, rows):
        nonlocal r
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 64)
        x[r:r + len(rows)] = rows
        names[name] = slice(r, r + len(rows))
        r += len(rows)

    put("all equal", [np.full(64, v) for v in (1.0, 0.1, 1e-310, 3e200, -2.5, 0.0, -0.0)])
    huge = 10.0 ** rng.uniform(-300.0, -250.0, (64, 64))
    huge[np.arange(64), np.arange(64)] = 1e300 * (1.0 + rng.random(64))
    put("one huge value at every lane", huge)
    put("one huge value at every lane, negative tiny ones", np.where(np.eye(64) > 0, huge, -huge))
    z = np.zeros((8, 64))
    z[0, ::2] = -0.0; z[1, 1::2] = -0.0; z[2, :20] = -0.0; z[3, 20:] = -0.0
    z[4] = rng.choice([0.0, -0.0, 5e-324, -5e-324, 2e-308, -2e-308], 64)
    z[5] = rng.choice([0.0, -0.0], 64)
    z[6] = rng.choice([5e-324, 1e-310, 2.2e-308, 0.0], 64)
    z[7] = -z[6]
    put("zeros of both signs and denormals", z)
    inf = 10.0 ** rng.uniform(-5.0, 5.0, (66, 64))
    inf[np.arange(64), np.arange(64)] = np.inf
    inf[64, :] = np.inf
    inf[65, 7] = np.inf; inf[65, 50] = np.inf
    put("+inf", inf)
    mixed = 10.0 ** rng.uniform(-20.0, 20.0, (400, 64)) * rng.choice([-1.0, 1.0], (400, 64))
    put("mixed signs", mixed)
    near = 1.0 + rng.random((400, 64))
    put("near-equal magnitudes", near)
    rest = K - r
    spread = np.repeat([[5.0], [40.0], [150.0], [300.0]], (rest + 3) // 4, axis=0)[:rest]
    put("positive weights over up to 600 decades", 10.0 ** (rng.uniform(-1.0, 1.0, (rest, 64)) * spread) * (1.0 + rng.random((rest, 64))))
    assert r == K and not np.isnan(x).any()
    return x, names


def _ints():
    rng = np.random.default_rng(142)
    x = rng.integers(I32.min, I32.max, (K, 64), endpoint=True)
    x[:1000] = rng.integers(-3, 3, (1000, 64))                                   # ties
    x[1000:1064] = 0; x[np.arange(1000, 1064), np.arange(64)] = I32.min           # INT_MIN at every lane
    x[1064:1128] = 0; x[np.arange(1064, 1128), np.arange(64)] = I32.max           # INT_MAX at every lane
    x[1128] = I32.min; x[1129] = I32.max; x[1130] = 7
    x[1131:1200] = rng.choice([I32.min, I32.max, 0, -1], (69, 64))
    # what the parent search feeds the butterfly: a chunk index in the active lanes, the neutral elements in the others
    act = rng.random((400, 64)) < 0.6
    x[1200:1600] = np.where(act, rng.integers(0, 157, (400, 64)), I32.max)
    x[1600:2000] = np.where(act, rng.integers(0, 157, (400, 64)), -1)
    return x.astype(np.int32)


@pytest.fixture(scope="module")
def probe(hiplib):
    from smcsmc_amd import pf
    xd, names = _doubles()
    xi = _ints()
    od, oi = pf.probe_wave_prims(xd, xi)
    return xd, xi, names, od, oi


def test_double_forms_agree_bit_for_bit(probe):
    from smcsmc_amd import pf
    xd, _, names, od, _ = probe
    ob = od.view(np.uint64)
    for j, prim in enumerate(pf.WAVE_PRIMS_D):
        for name, rows in names.items():
            bad = np.argwhere(ob[0, j, rows] != ob[1, j, rows])
            assert len(bad) == 0, "%s, %s: %d lanes differ, first (wavefront, lane) %s: %r against %r" % (
                prim, name, len(bad), bad[0], od[0, j, rows][tuple(bad[0])], od[1, j, rows][tuple(bad[0])])


def test_lds_forms_are_the_canonical_ones(probe):
    """the reference side of the comparison is what the oracle computes: the butterfly and the Hillis-Steele scan, in numpy"""
    xd, xi, _, od, oi = probe
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = xd.copy()
        for m in (1, 2, 4, 8, 16, 32):
            v = v + v[:, lanes ^ m]
        s = xd.copy()
        for d in (1, 2, 4, 8, 16, 32):
            s = np.where(lanes >= d, s[:, np.maximum(lanes - d, 0)] + s, s)
    ok = ~np.isnan(v)                      # (+inf and -huge never meet, but inf - inf would be a NaN: not compared)
    assert (od[0, 0].view(np.uint64)[ok] == v.view(np.uint64)[ok]).all()
    ok = ~np.isnan(s)
    assert (od[0, 1].view(np.uint64)[ok] == s.view(np.uint64)[ok]).all()
    assert (oi[0, 0] == np.maximum.accumulate(xi, axis=1)).all()
    assert (oi[0, 1] == xi.min(axis=1, keepdims=True)).all() and (oi[0, 2] == xi.max(axis=1, keepdims=True)).all()
    assert (oi[0, 3][:, 1:] == xi[:, :-1]).all() and (oi[0, 3][:, 0] == xi[:, 0]).all()


def test_integer_forms_agree(probe):
    from smcsmc_amd import pf
    _, _, _, _, oi = probe
    for j, prim in enumerate(pf.WAVE_PRIMS_I):
        bad = np.argwhere(oi[0, j] != oi[1, j])
        assert len(bad) == 0, "%s: %d lanes differ, first (wavefront, lane) %s" % (prim, len(bad), bad[0])


_ORACLE_RUNS = {}


def _oracle_run(oracle, Np):
    """model, segments and what the oracle makes of them, once per particle count and left unchanged"""
    if Np not in _ORACLE_RUNS:
        model = cases.make_model(n=4, E=10, L=1.5e5)
        segs = cases.make_segments(model, seed=24, max_seg_len=4000)
        o = oracle.Oracle(model, Np, seed=9, max_trace_events=64)
        o.init_prior(segs["start"][0])
        o.run(o.pack_segments(model, segs))
        _ORACLE_RUNS[Np] = (model, segs, o.trace(), o.resample_events(), o.particles(), o.logl())
        o.close()
    return _ORACLE_RUNS[Np]


@pytest.mark.parametrize("debug", [0, NO_SPEC_STAGE])
@pytest.mark.parametrize("Np", [4200, 8250])
def test_sweep_with_a_second_level_of_partials(oracle, hiplib, Np, debug):
    from smcsmc_amd import ParticleFilter
    nc = (Np + 63) // 64
    assert nc > 64 and Np % 64 != 0
    model, segs, to, (so, po), ps_o, logl_o = _oracle_run(oracle, Np)
    # the comparison of test_gpu_row_chain._against_oracle: trace, resampling parents, final particles, log-likelihood
    g = ParticleFilter(model, Np, seed=9, max_trace_events=64, debug=debug, local_recomb=True)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    g.run(); g.finish()
    tg = g.trace()
    assert g.segments_done() == len(to["T"])
    assert int(to["resampled"].sum()) >= 3, "the case does not resample: it checks nothing of decide_row's table or the parent search"
    assert (to["resampled"] == tg["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    sg, pg = g.resample_events()
    assert len(so) >= 3
    assert (so == sg).all() and (po == pg).all()
    ps_g = g.particles()
    assert (ps_o["children"] == ps_g["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(ps_o[k]) == _bits(ps_g[k])).all(), k
    assert _bits([logl_o])[0] == _bits([g.logl()])[0]
    g.close()
