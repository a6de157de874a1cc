"""The runs with ancient samples (model key sample_times) on which tests/test_gpu_ancient_parity.py compares the device with the oracle,
kept here so that tests/test_oracle_ancient_cpu.py can check without a device what those comparisons rely on: every run resamples, the
times move the result, and the edge a case is there for does occur.

Model: cases.make_model(E=8) and cases.make_structured(split_epoch=5); data from cases.make_segments on the base model (the site simulator
takes no sample times, and bit parity needs no matched data).  Times are given as the epoch at whose start each sample enters.  A sample
that enters after the join at epoch 5 is put into population 0 (nobody leaves a population that has been emptied for good), except in the
case "6-2-join", which is about entering at the join itself and keeps the migration rates positive from epoch 5 on."""
import functools

import numpy as np

import cases

E, SPLIT = 8, 5


def _groups(n, epochs=(0, 2, 4)):
    """n samples in len(epochs) groups of as equal a size as possible, the first the largest"""
    k = len(epochs)
    size = [n // k + (1 if g < n % k else 0) for g in range(k)]
    return [e for e, s in zip(epochs, size) for _ in range(s)]


# id, n, P, entry epoch per sample, particles, sequence length, seed (data and filter), 4 N0 m
CASES = [
    dict(id="2-2", n=2, P=2, epochs=[0, 2], Np=256, L=1.0e5, seed=2, mig=1.0, edge="alone_below"),
    dict(id="4-2", n=4, P=2, epochs=[0, 0, 2, 4], Np=256, L=1.0e5, seed=4, mig=1.0, edge="node_below"),
    dict(id="5-2-root-wait", n=5, P=2, epochs=[0, 0, 6, 6, 6], Np=256, L=8.0e4, seed=5, mig=1.0, pops=[0, 1, 0, 0, 0], edge="root_wait"),
    dict(id="6-2-join", n=6, P=2, epochs=[0, 0, 0, 5, 5, 5], Np=256, L=8.0e4, seed=6, mig=1.0, late_mig=True, edge="enter_at_join"),
    dict(id="7-3", n=7, P=3, epochs=_groups(7), Np=256, L=8.0e4, seed=7, mig=1.0, edge="node_below"),
    dict(id="8-4", n=8, P=4, epochs=_groups(8), Np=256, L=8.0e4, seed=8, mig=1.0, edge="node_below"),
    dict(id="9-2", n=9, P=2, epochs=_groups(9, (0, 3)), Np=200, L=6.0e4, seed=9, mig=1.0, edge="node_below"),
    dict(id="16-2", n=16, P=2, epochs=_groups(16), Np=192, L=6.0e4, seed=16, mig=1.0, edge="node_below"),
    dict(id="12-3", n=12, P=3, epochs=_groups(12), Np=192, L=6.0e4, seed=12, mig=1.0, edge="node_below"),
    dict(id="6-6", n=6, P=6, epochs=[0, 0, 0, 2, 2, 4], Np=256, L=8.0e4, seed=66, mig=2.0, edge="node_below"),
    dict(id="8-8", n=8, P=8, epochs=_groups(8), Np=256, L=8.0e4, seed=88, mig=2.0, edge="node_below"),
    dict(id="12-5", n=12, P=5, epochs=_groups(12), Np=192, L=6.0e4, seed=125, mig=2.0, edge="node_below"),
    dict(id="16-8", n=16, P=8, epochs=_groups(16), Np=192, L=6.0e4, seed=168, mig=1.0, edge="node_below"),
]
IDS = [c["id"] for c in CASES]
# the variants run on one narrow (P <= 4) and one wide (P > 4) case
VARIANT_CASES = ["8-4", "6-6"]
VARIANTS = ["missing-unphased", "vb", "local_map", "no-fuse"]


def by_id(case_id):
    return [c for c in CASES if c["id"] == case_id][0]


@functools.lru_cache(maxsize=None)
def inputs(case_id, variant=None):
    """(model, packed rows) of a case; the model carries sample_times"""
    c = by_id(case_id)
    n, P = c["n"], c["P"]
    base = cases.make_model(n=n, E=E, L=c["L"])
    kw = {}
    if variant == "missing-unphased":
        kw = dict(unphased=True, missing_block=(0.25 * c["L"], 0.5 * c["L"], list(range(n - 2, n))))
    segs = cases.make_segments(base, seed=c["seed"], max_seg_len=5000, **kw)
    model = cases.make_structured(base, P=P, split_epoch=SPLIT, mig=c["mig"], sample_pops=c.get("pops"))
    if c.get("late_mig"):
        mr = model["mig_rates"].copy()
        for e in range(SPLIT, E):
            mr[e] = mr[0]
        model["mig_rates"] = mr
    ct = model["change_times"]
    model["sample_times"] = [float(ct[e]) for e in c["epochs"]]
    if variant == "vb":
        rng = np.random.default_rng(c["seed"])
        model.update(vb_coal_counts=rng.uniform(0.5, 40.0, (E, P)), vb_mig_counts=rng.uniform(0.5, 40.0, (E, P, P)))
    return model, segs


def without_times(model):
    return dict(model, sample_times=[0.0] * model["nsam"])


CALIBRATION_POPS = [2, 6]


def calibration_model(P):
    """six samples in three groups for a lag calibration.  Its cost is the 16 384 trees of one batch on either side, whatever the sequence
    length (a replicate ends at 0.6 L or when its first tree's nodes are gone); what can be kept small is the number of migration events a
    tree collects, hence 4 N0 m = 0.5 at six populations."""
    base = cases.make_model(n=6, E=E, L=5e4)
    model = cases.make_structured(base, P=P, split_epoch=SPLIT, mig=1.0 if P == 2 else 0.5)
    model["sample_times"] = [float(model["change_times"][e]) for e in (0, 0, 0, 2, 2, 4)]
    return model


def _result(o, model, local_map):
    r = dict(trace=o.trace(), events=o.resample_events(), particles=o.particles(), migrations=o.migrations(), counts=o.counts(),
             logl=o.logl())
    if local_map:
        r["local_recomb"] = o.local_recomb(model["loci_length"])
    return r


@functools.lru_cache(maxsize=None)
def oracle_run(case_id, variant=None, zero=False):
    """the oracle's sweep of a case (zero: with every time set to 0), what the comparisons read"""
    import oracle_lib
    c = by_id(case_id)
    model, segs = inputs(case_id, variant)
    if zero:
        model = without_times(model)
    o = oracle_lib.Oracle(model, c["Np"], ess_fraction=0.5, seed=c["seed"], max_trace_events=64)
    if variant == "local_map":
        o.enable_local_recomb()
    o.init_prior(segs["start"][0])
    o.run(o.pack_segments(model, segs))
    r = _result(o, model, variant == "local_map")
    o.close()
    return r


@functools.lru_cache(maxsize=None)
def oracle_prior(case_id):
    """particles and migration lists after init_prior alone: the first trees"""
    import oracle_lib
    c = by_id(case_id)
    model, segs = inputs(case_id)
    o = oracle_lib.Oracle(model, c["Np"], ess_fraction=0.5, seed=c["seed"], max_trace_events=0)
    o.init_prior(segs["start"][0])
    r = dict(particles=o.particles(), migrations=o.migrations())
    o.close()
    return r


def mrca_height(particles, n, a, b):
    """height of the youngest node above both samples a and b, per particle"""
    H, Ch = particles["heights"], particles["children"].astype(int)
    Np = len(H)
    rows = np.arange(Np)
    below = np.zeros((Np, 2 * n - 1), np.int64)
    below[:, :n] = 1 << np.arange(n)
    out = np.full(Np, np.nan)
    want = (1 << a) | (1 << b)
    for r in range(n - 1):
        below[:, n + r] = below[rows, Ch[:, r, 0]] | below[rows, Ch[:, r, 1]]
        hit = ((below[:, n + r] & want) == want) & np.isnan(out)
        out[hit] = H[hit, r]
    return out


def edge_measure(case_id):
    """(description, number of particles of the oracle's first trees in which the case's edge occurs, of how many)"""
    c = by_id(case_id)
    model, _ = inputs(case_id)
    n = c["n"]
    pr = oracle_prior(case_id)
    H = pr["particles"]["heights"]
    mg = pr["migrations"]
    tau = np.array(model["sample_times"])
    ct = model["change_times"]
    Np = len(H)
    kind = c["edge"]
    if kind == "alone_below":
        # sample 0 is alone below the time of sample 1: the only node lies above it, and the interval below it carries one lineage
        return "one-node trees whose node lies above the time of sample 1 (k = 1 below it)", int((H[:, 0] > tau[1]).sum()), Np
    if kind == "root_wait":
        # the root of the first two samples below the time at which the third enters: its lineage waits for it
        h01 = mrca_height(pr["particles"], n, 0, 1)
        usually = int((h01 < tau[2]).sum())
        crosses = int((h01 < ct[SPLIT]).sum())
        assert usually > Np // 2, "the root of the first two samples is usually below the next entry time: %d of %d" % (usually, Np)
        assert model["mig_rates"][SPLIT - 1].sum() > 0
        return "root of samples 0, 1 below the entry at T[6] in %d; its wait crosses the join at T[5] in" % usually, crosses, Np
    if kind == "enter_at_join":
        # samples enter in population 1 at the very epoch start that moves population 1 to 0: the move is not theirs
        late = [i for i in range(n) if tau[i] == ct[SPLIT]]
        assert late and all(model["sample_pops"][i] == 1 for i in late) and model["single_mig"][SPLIT, 1, 0] == 1.0
        moved = 0
        for i in range(Np):
            k = mg["n_events"][i]
            at = mg["times"][i, :k] == ct[SPLIT]
            assert not np.isin(mg["branch"][i, :k][at], late).any(), "an event on an entering sample's branch at the join"
            moved += bool(at.any())
        stay = sum(1 for i in range(Np) if any(mg["branch"][i, m] in late for m in range(mg["n_events"][i])))
        assert stay > 0, "no entering sample ever leaves population 1 by migration"
        return "trees with a move at T[5] on another lineage, none on an entering sample's (which migrate out later in %d)" % stay, moved, Np
    # node_below: an internal node below the latest entry time, so the lineage count of an interval is samples entered minus nodes passed
    cnt = int((H[:, 0] < tau.max()).sum())
    return "first trees with a node below the latest entry time", cnt, Np
