"""The runs on which tests/test_gpu_emission_flags.py compares the device with the oracle under the two model flags that enter the weight
of a site: dephase (every heterozygous pair counts as unphased) and ancestral_aware (root prior 1, 0).  The mean over phasings is written
out seven times in device code; CASES names, for every copy, the smallest run that reaches it, and what run_path() / row_form() must say.

Data: cases.make_segments(unphased=False) with one whole pair missing over a quarter of the sequence; then, in every third site row, the
heterozygous pairs become marks (2, 2) -- in every other such row all but the last, so that marks and phased pairs meet in one row.
rows() asserts what the data must contain before anything runs (PROPERTIES), so that a case cannot pass by not exercising the code, and
that no row has more than MAX_PAIRS pairs to enumerate: the oracle's cost per site is 2^pairs site likelihoods per particle.  `seed` picks
the simulated data set; it was chosen among the first few for few heterozygous pairs at the busiest site (as in wide_cases.py)."""
import functools

import numpy as np

import cases

MAX_PAIRS = 10
NO_FUSE, NO_PAIR = 2, 4096
FLAGS = {"dephase": dict(dephase=True), "ancestral_aware": dict(ancestral_aware=True), "both": dict(dephase=True, ancestral_aware=True)}

# shape: n, P, E, L, particles, max_seg_len, data seed (also the filter's).  Variants of one shape share the oracle's run.
SHAPES = {
    "4":    dict(n=4, P=1, E=8, L=6.0e4, Np=300, msl=5000, seed=1),
    "7":    dict(n=7, P=1, E=8, L=6.0e4, Np=256, msl=5000, seed=5),
    "9":    dict(n=9, P=1, E=8, L=6.0e4, Np=256, msl=5000, seed=5),
    "33":   dict(n=33, P=1, E=8, L=1.2e4, Np=100, msl=2000, seed=11),
    "9-2":  dict(n=9, P=2, E=6, L=6.0e4, Np=200, msl=5000, seed=5),
    "5-5":  dict(n=5, P=5, E=6, L=6.0e4, Np=256, msl=5000, seed=3),
    "6-2-ancient": dict(n=6, P=2, E=8, L=6.0e4, Np=256, msl=5000, seed=11, ancient="6-2-join"),
    "4-2":  dict(n=4, P=2, E=6, L=6.0e4, Np=320, msl=5000, seed=6),
    "6-3":  dict(n=6, P=3, E=6, L=6.0e4, Np=300, msl=5000, seed=11),
}

# id, shape, copy of the averaging it reaches, constructor arguments, how it runs, the path and the row form it must report
CASES = [
    dict(id="4-single", shape="4", copy=1, kw=dict(debug=NO_PAIR), how="run", path="SweepSplit", form="single", kernel="k_sweep4"),
    dict(id="4-paired", shape="4", copy=2, kw=dict(), how="run", path="SweepSplit", form="paired", kernel="k_sweep4p"),
    dict(id="7-sweep", shape="7", copy=1, kw=dict(), how="run", path="Sweep", form=None, kernel="k_sweep"),
    dict(id="7-no-fuse", shape="7", copy=1, kw=dict(debug=NO_FUSE), how="run", path="General", form=None, kernel="k_extend_reg"),
    dict(id="9-general", shape="9", copy=3, kw=dict(), how="run", path="General", form=None, kernel="k_extend"),
    dict(id="33-wide", shape="33", copy=3, kw=dict(), how="run", path="General", form=None, kernel="k_extend_wide"),
    dict(id="9-lockstep", shape="9", copy=4, kw=dict(), how="many", path="SweepXl", form=None, kernel="k_sweep_xl"),
    dict(id="9-2-general", shape="9-2", copy=5, kw=dict(), how="run", path="General", form=None, kernel="k_extend_mp"),
    dict(id="5-5-wide-walk", shape="5-5", copy=5, kw=dict(), how="run", path="General", form=None, kernel="k_extend_mp (eight counters)"),
    dict(id="6-2-ancient", shape="6-2-ancient", copy=5, kw=dict(), how="run", path="General", form=None, kernel="k_extend_mp (PF_ANC)"),
    dict(id="4-2-no-fuse", shape="4-2", copy=6, kw=dict(debug=NO_FUSE), how="run", path="General", form=None, kernel="k_extend_mpr"),
    dict(id="6-3-rows", shape="6-3", copy=6, kw=dict(), how="run", path="SweepXmp", form=None, kernel="k_sweep_xmp"),
    dict(id="9-2-rows", shape="9-2", copy=7, kw=dict(mp_rows=True), how="run", path="SweepXlmp", form=None, kernel="k_sweep_xlmp"),
]
IDS = [c["id"] for c in CASES]
PROPERTIES = ("het01", "het10", "mark_and_het", "two_dephased", "het_beside_missing", "derived_on_last")


def by_id(case_id):
    return [c for c in CASES if c["id"] == case_id][0]


def is_het(a, b):
    return (a == 0 and b == 1) or (a == 1 and b == 0)


def mark_rows(segs, n):
    """the marks: see the module's docstring.  Only site rows (state 0) change; no row gains or loses a missing sample."""
    al = np.array(segs["alleles"], np.int8).reshape(len(segs["start"]), n)
    sites = np.nonzero(np.asarray(segs["state"]) == 0)[0]
    for k, s in enumerate(sites[::3]):
        het = [i for i in range(0, n - 1, 2) if is_het(al[s, i], al[s, i + 1])]
        if k % 2 == 1 and len(het) >= 2:
            het = het[:-1]
        for i in het:
            al[s, i] = al[s, i + 1] = 2
    return dict(segs, alleles=al)


def measure(segs, n):
    """(which of PROPERTIES hold in some site row, most pairs to enumerate under dephase in one row)"""
    al = np.asarray(segs["alleles"]).reshape(len(segs["start"]), n)
    have = dict.fromkeys(PROPERTIES, False)
    most = 0
    for s in np.nonzero(np.asarray(segs["state"]) == 0)[0]:
        pairs = [(int(al[s, i]), int(al[s, i + 1])) for i in range(0, n - 1, 2)]
        marks = sum(1 for a, b in pairs if a == 2 and b == 2)
        hets = sum(1 for a, b in pairs if is_het(a, b))
        gone = sum(1 for a, b in pairs if a == -1 and b == -1)
        assert all((a == 2) == (b == 2) for a, b in pairs) and (n % 2 == 0 or al[s, n - 1] != 2), "a lone mark"
        most = max(most, marks + hets)
        have["het01"] |= (0, 1) in pairs
        have["het10"] |= (1, 0) in pairs
        have["mark_and_het"] |= marks >= 1 and hets >= 1
        have["two_dephased"] |= hets >= 2
        have["het_beside_missing"] |= gone >= 1 and marks + hets >= 1
        have["derived_on_last"] |= n % 2 == 1 and al[s, n - 1] == 1
    if n % 2 == 0:
        have["derived_on_last"] = True          # (no unpaired sample)
    return have, most


def make_rows(n, E, L, seed, msl):
    base = cases.make_model(n=n, E=E, L=L)
    segs = cases.make_segments(base, seed=seed, unphased=False, max_seg_len=msl, missing_block=(0.25 * L, 0.5 * L, (2, 3)))
    return base, mark_rows(segs, n)


@functools.lru_cache(maxsize=None)
def rows(shape):
    """(one-population model the data were drawn from, packed rows) of a shape, the data's conditions asserted"""
    s = SHAPES[shape]
    base, segs = make_rows(s["n"], s["E"], s["L"], s["seed"], s["msl"])
    have, most = measure(segs, s["n"])
    missing = [k for k in PROPERTIES if not have[k]]
    assert not missing, "shape %s: no site row with %s" % (shape, missing)
    assert most <= MAX_PAIRS, "shape %s: a row with %d pairs to enumerate" % (shape, most)
    return base, segs


def model(shape, flags=None):
    """the model of a shape under a flag setting (a key of FLAGS, or None for neither)"""
    s = SHAPES[shape]
    base, _ = rows(shape)
    if s.get("ancient"):
        import ancient_cases
        m = dict(ancient_cases.inputs(s["ancient"])[0], loci_length=base["loci_length"])
        assert m["nsam"] == s["n"] and m["n_pops"] == s["P"] and len(m["change_times"]) == s["E"] and max(m["sample_times"]) > 0
    elif s["P"] > 1:
        m = cases.make_structured(base, P=s["P"], split_epoch=s["E"] - 3, mig=1.0)
    else:
        m = base
    return dict(m, **(FLAGS[flags] if flags else {}))


def _result(o, P):
    r = dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), counts=o.counts(), logl=o.logl())
    if P > 1:
        r["migrations"] = o.migrations()
    return r


@functools.lru_cache(maxsize=None)
def oracle_run(shape, flags=None, lookahead=0):
    """the oracle's sweep of a shape under a flag setting, what the comparisons read; computed once and left unchanged.  lookahead: the
    level of the auxiliary particle filter (tables of lookahead_inputs)"""
    import oracle_lib
    s = SHAPES[shape]
    m = model(shape, flags)
    _, segs = rows(shape)
    o = oracle_lib.Oracle(m, s["Np"], ess_fraction=0.5, seed=s["seed"], max_trace_events=64)
    o.init_prior(segs["start"][0])
    si = o.pack_segments(m, segs)
    if lookahead:
        la, tbl = lookahead_inputs(shape)
        o.load_lookahead(la, lookahead, tbl)
    o.run(si)
    r = _result(o, s["P"])
    o.close()
    return r


# ---- the look-ahead under dephase: "dephase ... (but use phasing for -apf)"
SHAPES["8-apf"] = dict(n=8, P=1, E=8, L=6.0e4, Np=320, msl=5000, seed=1)
APF_LEVEL = 2


@functools.lru_cache(maxsize=None)
def lookahead_inputs(shape):
    """(look-ahead records of the rows as they are phased, terminal-branch quantile table from the oracle)"""
    import oracle_lib
    from smcsmc_amd import segments as segmod
    s = SHAPES[shape]
    base, segs = rows(shape)
    recs = [(int(a) + 1, int(b), int(st), list(map(int, al)))
            for a, b, st, al in zip(segs["start"], segs["length"], segs["state"], np.asarray(segs["alleles"]).reshape(-1, s["n"]))]
    la = segmod.pack_lookahead(recs, s["n"])
    assert (la["n_doubletons"] > 0).any()
    return la, oracle_lib.terminal_branch_quantiles(base, seed=1, n_trees=20000)


# ---- the identity that needs no oracle: dephase on phased rows == no flag on the same rows with every heterozygous pair marked
IDENTITY_SHAPES = ["4", "7", "4-2", "9"]


@functools.lru_cache(maxsize=None)
def identity_rows(shape):
    """(phased rows, the same rows with every phased heterozygous pair rewritten as (2, 2)); the missing block stays.  Asserted: pairs in
    either order, and rows with two or more of them (the carry of the enumeration)."""
    s = SHAPES[shape]
    n = s["n"]
    base = cases.make_model(n=n, E=s["E"], L=s["L"])
    segs = cases.make_segments(base, seed=s["seed"], unphased=False, max_seg_len=s["msl"], missing_block=(0.25 * s["L"], 0.5 * s["L"], (2, 3)))
    have, most = measure(segs, n)
    assert have["het01"] and have["het10"] and have["two_dephased"] and have["het_beside_missing"] and most <= MAX_PAIRS
    al = np.array(segs["alleles"], np.int8).reshape(len(segs["start"]), n)
    assert not (al == 2).any()
    for i in range(0, n - 1, 2):
        het = (np.asarray(segs["state"]) == 0) & (al[:, i] >= 0) & (al[:, i + 1] >= 0) & (al[:, i] != al[:, i + 1])
        al[het, i] = 2
        al[het, i + 1] = 2
    return segs, dict(segs, alleles=al)


@functools.lru_cache(maxsize=None)
def identity_oracle(shape, marked):
    """the oracle on the phased rows with dephase (marked=False), or on the marked rows without (marked=True)"""
    import oracle_lib
    s = SHAPES[shape]
    m = model(shape, None if marked else "dephase")
    segs = identity_rows(shape)[1 if marked else 0]
    o = oracle_lib.Oracle(m, s["Np"], ess_fraction=0.5, seed=s["seed"], max_trace_events=64)
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(m, segs))
    r = _result(o, s["P"])
    o.close()
    return r
