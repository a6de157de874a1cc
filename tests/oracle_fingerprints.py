"""Fingerprints of the CPU oracle at 2..16 haplotypes: the configurations and what is recorded of each run.

tests/golden/oracle_fingerprints.json holds them as recorded with the oracle of the commit BEFORE its capacity went from 16 to 64
haplotypes (tests/golden/make_oracle_fingerprints.py writes the file); tests/test_oracle_wide_cpu.py recomputes them with the
oracle as built and compares for equality.  Floating-point results are kept as the hex bit patterns of the doubles, integer
arrays (resampling parents, children, tree events) as SHA-256 of their bytes.  Everything runs on the CPU."""
import hashlib

import numpy as np

import cases

COUNT_KEYS = ("coal_count", "coal_opp", "coal_weight", "rec_count", "rec_opp", "rec_weight")


def hexbits(a):
    """the bit patterns of an array of doubles, 16 hex digits each"""
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64).reshape(-1)
    return ["%016x" % v for v in a.view(np.uint64)]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def _biased(E, delay_type):
    return dict(bias_heights=[400.0], bias_strengths=[3.0, 1.0], delay_type=delay_type, application_delays=np.full(E, 3000.0))


def _lookahead_rows(segs):
    return [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]


# name -> (kind, n, E, Np, L): about ten runs spread over n = 2..16
CONFIGS = [
    ("plain_n2", "plain", 2, 1, 200, 8e4),
    ("plain_n5", "plain", 5, 8, 150, 6e4),
    ("biased_delay0_n7", "biased0", 7, 8, 120, 6e4),
    ("biased_delay1_n12", "biased1", 12, 6, 100, 5e4),
    ("guide_bias_n6", "guide", 6, 6, 120, 6e4),
    ("unphased_missing_n8", "unphased", 8, 8, 120, 6e4),
    ("local_map_n9", "local_map", 9, 8, 100, 6e4),
    ("two_pops_join_n10", "two_pops", 10, 6, 80, 4e4),
    ("apf2_unphased_n4", "apf2", 4, 8, 150, 6e4),
    ("tree_recording_n6", "trees", 6, 6, 100, 5e4),
    ("plain_n16", "plain", 16, 16, 100, 4e4),
    ("calibration_n16", "calibration", 16, 8, 0, 5e6),
]


def fingerprint(oracle_lib, name):
    """runs configuration `name` on the oracle behind `oracle_lib` and returns what the fixture keeps of it"""
    _, kind, n, E, Np, L = [c for c in CONFIGS if c[0] == name][0]
    model = cases.make_model(n=n, E=E, L=L)
    if kind == "calibration":
        med, trees = oracle_lib.median_survival(model, seed=1, min_events=50, max_trees=32768)
        return dict(kind=kind, n=n, trees=int(trees), medians=hexbits(med))
    seed = 40 + n
    data_model = model
    if kind == "biased0":
        model = dict(model, **_biased(E, 0))
    elif kind == "biased1":
        model = dict(model, **_biased(E, 1))
    elif kind == "guide":
        model = dict(model, guide=cases.guide(model, 9, 2.5, n), **_biased(E, 0))
    elif kind == "two_pops":
        model = cases.make_structured(model, P=2, split_epoch=4, mig=2.0)
    segs = cases.make_segments(data_model, seed=seed, max_seg_len=5000, unphased=kind in ("unphased", "apf2"),
                               missing_block=(20000, 35000, (n - 2, n - 1)) if kind in ("unphased", "apf2") else None)
    o = oracle_lib.Oracle(model, Np, seed=n, max_trace_events=64)
    if kind == "local_map":
        o.enable_local_recomb()
    if kind == "trees":
        o.enable_tree_recording()
    o.init_prior(segs["start"][0])
    if kind == "apf2":
        from smcsmc_amd import segments as segmod
        tbl = oracle_lib.terminal_branch_quantiles(model, seed=1, n_trees=20000)
        o.load_lookahead(segmod.pack_lookahead(_lookahead_rows(segs), n), 2, tbl)
    o.run(o.pack_segments(model, segs))
    tr, c, p = o.trace(), o.counts(), o.particles()
    seg_idx, parents = o.resample_events()
    out = dict(kind=kind, n=n, rows=int(len(tr["T"])), resamplings=int(tr["resampled"].sum()),
               logl=hexbits(o.logl())[0],
               trace={k: hexbits(tr[k]) for k in ("T", "ess", "logl")},
               resampled=sha(tr["resampled"]), parents=sha(seg_idx, parents),
               counts={k: hexbits(c[k]) for k in COUNT_KEYS},
               particles=dict(children=sha(p["children"]), **{k: sha(hexbits(p[k])) for k in ("heights", "w_post", "w_pilot", "next_base")}))
    if "mig_count" in c:
        out["counts"].update({k: hexbits(c[k]) for k in ("mig_count", "mig_opp", "mig_weight")})
    if kind == "local_map":
        lm = o.local_recomb(L)
        out["local_map"] = dict(opp_diff=sha(hexbits(lm["opp_diff"])), counts=sha(hexbits(lm["counts"])),
                                per_sample=hexbits(lm["counts"][:n].sum(axis=1)))
    if kind == "trees":
        part, ek, pos, hgt, desc = o.sample_tree_events()
        out["tree_events"] = dict(particle=int(part), n=int(len(ek)), kind=sha(ek), desc=sha(desc.astype(np.uint64)),
                                  pos=sha(hexbits(pos)), height=sha(hexbits(hgt)))
    o.close()
    return out
