"""The by-case form of a genealogy update's integer part at four haplotypes (r4_select / r4_edit, pf_tree_reg.h), which the
row kernel k_sweep4<EXACT> runs in place of the loops written for any number of haplotypes.

(a) Both forms side by side on the device (pf_probe_tree_edit), on every four-leaf tree, every cut branch, every interval the
    cut point and the coalescence time can fall into, and every re-attachment the uniform can pick: the outputs are equal.
(b) Sweeps through the default path against the oracle, bit for bit, with the counts and the local recombination map (what the
    descendant mask of the selection feeds) within the tolerance of the existing parity tests.
(c) A path that keeps the general form (three haplotypes in the four-haplotype kernel), bit for bit."""
import itertools

import numpy as np
import pytest

import cases

NO_DRAW_TABLE = 128          # PF_DEBUG_NO_DRAW_TABLE: every update computes its own uniforms (Philox) instead of reading the table
HEIGHTS = (0.37, 1.21, 2.9)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- (a) the enumeration

def all_trees():
    """The 18 ranked labelled histories of four leaves x the 8 orders of the children within the nodes, as (C[3][2], leaves below
    each node id, topology number).  Node of rank r has id 4 + r."""
    out = []
    topo = 0
    for a in itertools.combinations(range(4), 2):
        rest = [x for x in range(4) if x not in a] + [4]
        for b in itertools.combinations(rest, 2):
            c = tuple(x for x in rest if x not in b) + (5,)
            for flips in itertools.product((0, 1), repeat=3):
                ch = [tuple(reversed(p)) if f else tuple(p) for p, f in zip((a, b, c), flips)]
                below = {i: {i} for i in range(4)}
                for r in range(3):
                    below[4 + r] = below[ch[r][0]] | below[ch[r][1]]
                out.append((ch, below, topo))
            topo += 1
    assert len(out) == 144 and topo == 18
    return out


def _height(i):
    return 0.0 if i < 4 else HEIGHTS[i - 4]


def _lineages_at(ch, t):
    """the slots (rank, side) of the lineages at time t in the enumeration order of the kernels: rank ascending, child 0 then 1"""
    return [(r, s) for r in range(3) for s in (0, 1) if HEIGHTS[r] > t and _height(ch[r][s]) <= t]


def enumerate_cases():
    """One case per (tree, cut branch, interval of the cut point, interval of the coalescence time, re-attachment index)."""
    S, C, H, LIN, RP, SB, TC, U, TOPO = [], [], [], [], [], [], [], [], []
    for ch, below, topo in all_trees():
        for rp in range(3):
            for sb in (0, 1):
                b, s = ch[rp][sb], ch[rp][1 - sb]
                lo, Sp = _height(b), HEIGHTS[rp]
                # the cut point: the middle of every interval between node heights inside the branch, and the branch's lower end
                marks = [lo] + [x for x in HEIGHTS if lo < x < Sp] + [Sp]
                hs = [0.5 * (marks[i] + marks[i + 1]) for i in range(len(marks) - 1)]
                hs.append(lo)                            # h equal to a node height (or 0 for a leaf): the `<=` of the prefix count
                for h in hs:
                    lin = _lineages_at(ch, h).index((rp, sb))           # the one `lin` that selects this branch at this h
                    # the coalescence time: between h and the next node height, in every interval above, above the root ...
                    tmarks = [h] + [x for x in HEIGHTS if x > h]
                    tcs = [0.5 * (tmarks[i] + tmarks[i + 1]) for i in range(len(tmarks) - 1)] + [HEIGHTS[2] + 1.7]
                    tcs += [x for x in HEIGHTS if x >= h]               # ... and exactly at a node height
                    # what is left when p and everything below b are gone: leaves, and the nodes that join them
                    rem_leaves = 4 - len(below[b])
                    rem_nodes = [HEIGHTS[r] for r in range(3) if r != rp and not (4 + r == b or below[4 + r] < below[b])]
                    for tc in tcs:
                        k = rem_leaves - sum(1 for x in rem_nodes if x <= tc) + (1 if tc < Sp else 0)
                        assert 1 <= k <= 5
                        for j in range(k):                              # idx = int(u k) takes every value 0..k-1
                            S.append(HEIGHTS); C.append([ch[0][0], ch[0][1], ch[1][0], ch[1][1], ch[2][0], ch[2][1]])
                            H.append(h); LIN.append(lin); RP.append(rp); SB.append(sb); TC.append(tc); U.append((j + 0.5) / k)
                            TOPO.append(topo)
    return dict(S=np.array(S), C=np.array(C, np.int32), h=np.array(H), lin=np.array(LIN, np.int32), rp=np.array(RP, np.int32),
                sb=np.array(SB, np.int32), tc=np.array(TC), u=np.array(U), topo=np.array(TOPO))


def check_probe_outputs(cs, oi, od):
    """what test (a) asserts of the probe's outputs"""
    n = len(cs["h"])
    gen_i, spec_i, gen_d, spec_d = oi[0], oi[1], od[0], od[1]
    # the general form selects the branch the case was built for: the enumeration means what it says
    assert (gen_i[:, 0] == cs["rp"]).all() and (gen_i[:, 1] == cs["sb"]).all()
    names = ["rp", "sb", "last_desc", "C0[0]", "C1[0]", "C0[1]", "C1[1]", "C0[2]", "C1[2]", "changed"]
    for k, name in enumerate(names):
        bad = np.nonzero(gen_i[:, k] != spec_i[:, k])[0]
        assert len(bad) == 0, (name, len(bad), {q: cs[q][bad[0]] for q in ("S", "C", "h", "lin", "rp", "sb", "tc", "u")}, gen_i[bad[0]], spec_i[bad[0]])
    for k, name in enumerate(["S[0]", "S[1]", "S[2]", "Sp"]):
        bad = np.nonzero(_bits(gen_d[:, k]) != _bits(spec_d[:, k]))[0]
        assert len(bad) == 0, (name, len(bad), gen_d[bad[0]], spec_d[bad[0]])
    # every outcome occurs, read from the general form's outputs: back into its own branch (nothing changed), above the root (the
    # new node, at height tc, is the top rank) or onto a slot; each with the removed node the root or not, the cut branch above
    # a leaf or above a node
    changed = gen_i[:, 9] != 0
    own = ~changed
    above = changed & (_bits(gen_d[:, 2]) == _bits(cs["tc"]))
    slot = changed & ~above
    was_root = cs["rp"] == 2
    leaf = cs["C"][np.arange(n), 2 * cs["rp"] + cs["sb"]] < 4
    for oname, o in (("own branch", own), ("above the root", above), ("slot", slot)):
        for r in (False, True):
            for lf in (False, True):
                assert (o & (was_root == r) & (leaf == lf)).sum() > 0, (oname, r, lf)
    assert (_bits(gen_d[own, :3]) == _bits(cs["S"][own])).all() and (gen_d[own, 3] > cs["tc"][own]).all()
    # both sides of Sp, and a tc equal to a node height on every topology
    assert (cs["tc"] < gen_d[:, 3]).any() and (cs["tc"] > gen_d[:, 3]).any()
    tie = (cs["tc"][:, None] == cs["S"]).any(axis=1)
    assert set(cs["topo"][tie]) == set(range(18))


def test_enumeration_is_complete():
    cs = enumerate_cases()
    n = len(cs["h"])
    assert 20000 <= n <= 40000, n                  # a few tens of thousands: one launch of the probe
    keys = set(zip(map(tuple, cs["C"]), cs["rp"], cs["sb"]))
    assert len(keys) == 144 * 6
    assert len(set(cs["topo"])) == 18


@pytest.mark.gpu
def test_by_case_form_equals_general_form_on_every_case(hiplib):
    from smcsmc_amd import pf
    cs = enumerate_cases()
    oi, od = pf.probe_tree_edit(cs["S"], cs["C"], cs["h"], cs["lin"], cs["rp"], cs["sb"], cs["tc"], cs["u"])
    check_probe_outputs(cs, oi, od)


# ---------------------------------------------------------------- (b), (c) sweeps against the oracle

_ORACLE_RUNS = {}


def _oracle_run(oracle, key, model, segs, Np, seed):
    """the oracle's run of a case, computed once and shared (read only)"""
    if key not in _ORACLE_RUNS:
        o = oracle.Oracle(model, Np, seed=seed, max_trace_events=64)
        o.enable_local_recomb()
        o.init_prior(segs["start"][0])
        o.run(o.pack_segments(model, segs))
        _ORACLE_RUNS[key] = dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), logl=o.logl(), counts=o.counts(),
                                 updates=o.stats()["recombinations"], lmap=o.local_recomb(model["loci_length"]))
        o.close()
    return _ORACLE_RUNS[key]


def _case(name):
    n = 3 if name == "n3" else 4
    if name == "long_rows":
        # few sites and long rows: a lane does several updates in one row
        model = cases.make_model(n=n, E=10, L=1.5e5, mu=4e-9)
        segs = cases.make_segments(model, seed=24, max_seg_len=20000)
    else:
        model = cases.make_model(n=n, E=10, L=1.5e5)
        segs = cases.make_segments(model, seed=20 + n, max_seg_len=4000)
    return model, segs


def _against_oracle(oracle, name, Np, seed, **gpu_kw):
    from smcsmc_amd import ParticleFilter
    model, segs = _case(name)
    n = model["nsam"]
    ref = _oracle_run(oracle, (name, Np, seed), model, segs, Np, seed)
    g = ParticleFilter(model, Np, seed=seed, max_trace_events=64, local_recomb=True, **gpu_kw)
    g.init_prior(segs["start"][0]); g.load_segments(segs)
    g.run(); g.finish()
    to, tg = ref["trace"], g.trace()
    assert g.segments_done() == len(to["T"])
    assert (to["resampled"] == tg["resampled"]).all()
    for k in ("T", "ess", "logl"):
        assert (_bits(to[k]) == _bits(tg[k])).all(), k
    (so, po), (sg, pg) = ref["events"], g.resample_events()
    assert len(so) >= 3, "the case hardly resamples"
    assert (so == sg).all() and (po == pg).all()
    ps_o, ps_g = ref["particles"], g.particles()
    assert (ps_o["children"] == ps_g["children"]).all()
    for k in ("heights", "w_post", "w_pilot", "next_base"):
        assert (_bits(ps_o[k]) == _bits(ps_g[k])).all(), k
    assert _bits([ref["logl"]])[0] == _bits([g.logl()])[0]
    co, cg = ref["counts"], g.counts()
    for k in ("coal_count", "coal_opp", "rec_count", "rec_opp"):
        np.testing.assert_allclose(cg[k], co[k], rtol=1e-9, atol=1e-300, err_msg=k)
    # the local recombination map, its per-sample rows included (sums of the same terms in another order: the bound of the
    # existing comparisons of this array with the oracle)
    lo, lg = ref["lmap"], g.local_recomb()
    assert lo["counts"][:n].sum() > 0 and (lo["counts"][:n].sum(axis=1) > 0).all()
    np.testing.assert_allclose(lg["counts"], lo["counts"], rtol=1e-9, atol=1e-12 * lo["counts"].max())
    np.testing.assert_allclose(np.cumsum(lg["opp_diff"]), np.cumsum(lo["opp_diff"]), rtol=1e-9, atol=1e-9 * np.cumsum(lo["opp_diff"]).max())
    g.close()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,Np,debug", [("default", 300, 0), ("default", 1000, 0), ("long_rows", 300, 0), ("long_rows", 1000, 0),
                                           ("long_rows", 300, NO_DRAW_TABLE)])
def test_four_haplotype_sweep_equals_oracle(oracle, hiplib, name, Np, debug):
    assert Np % 64 != 0 and Np % 256 != 0
    ref = _against_oracle(oracle, name, Np, seed=9, debug=debug)
    if name == "long_rows":
        model, segs = _case(name)
        assert ref["updates"] > 2.5 * Np * len(segs["start"]), "the rows are too short for several updates per particle and row"


@pytest.mark.gpu
def test_three_haplotypes_in_the_same_kernel_keep_the_general_form(oracle, hiplib):
    _against_oracle(oracle, "n3", 300, seed=9)
