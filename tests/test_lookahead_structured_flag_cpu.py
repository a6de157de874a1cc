"""The opt-in of the look-ahead on the row pipeline of structured models, as far as it can be seen without a GPU: the Python wrapper
puts PF_LA_ROW_PIPELINE_MP (bit 1) into pf_lookahead.flags beside or without bit 0, the oracle, which has no such path, is still handed
0, and the help of bin/smcsmc says that -apf_pipeline covers structured models."""
import subprocess

import numpy as np

import cases
from smcsmc_amd import pf, segments as segmod


def _lookahead(n=4):
    base = cases.make_model(n=n, E=6, L=6e4)
    segs = cases.make_segments(base, seed=3, max_seg_len=5000)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return base, segs, segmod.pack_lookahead(rows, n)


def test_packed_lookahead_carries_the_structured_flag():
    assert pf.LA_ROW_PIPELINE_MP == 2 and pf.LA_ROW_PIPELINE == 1
    _, _, la = _lookahead()
    Q = segmod.TBL_QUANTILES
    tbl = (np.ones((4, len(Q))), 1.0)
    assert pf.PackedLookahead(la, 2, tbl, Q, structured=True).struct.flags == 2
    assert pf.PackedLookahead(la, 2, tbl, Q, pipeline=True, structured=True).struct.flags == 3
    assert pf.PackedLookahead(la, 2, tbl, Q, pipeline=True).struct.flags == 1
    assert pf.PackedLookahead(la, 2, tbl, Q, pipeline=False, structured=False).struct.flags == 0
    assert pf.PackedLookahead(la, 2, tbl, Q).struct.flags == 0
    s = pf.PackedLookahead(la, 4, tbl, Q, structured=True).struct          # the other fields are where they were
    assert (s.level, s.max_doubletons, s.n_quantiles, s.n) == (4, int(la["max_doubletons"]), len(Q), len(la["n_doubletons"]))


def test_load_lookahead_takes_the_keyword():
    import inspect
    par = inspect.signature(pf.ParticleFilter.load_lookahead).parameters
    assert par["structured"].default is False and par["pipeline"].default is False


def test_the_oracle_is_handed_no_flag_with_structure(oracle):
    base, segs, la = _lookahead()
    model = cases.make_structured(base, P=2, split_epoch=4, mig=1.5)
    o = oracle.Oracle(model, 64, seed=3)
    o.init_prior(segs["start"][0])
    si = o.pack_segments(model, segs)
    o.load_lookahead(la, 2, oracle.terminal_branch_quantiles(base, seed=1, n_trees=2000))
    assert o._la.struct.flags == 0
    o.run(si)
    assert np.isfinite(o.logl())


def test_the_help_of_apf_pipeline_mentions_structured_models(built_binary):
    r = subprocess.run([built_binary, "-help"], capture_output=True, text=True)
    text = r.stdout + r.stderr
    lines = text.splitlines()
    at = [i for i, ln in enumerate(lines) if "-apf_pipeline" in ln]
    assert at, "-apf_pipeline is not in the help"
    entry = " ".join(lines[at[0]:at[0] + 3])                                # (the table wraps long descriptions)
    assert "structured" in entry
