"""The opt-in of the look-ahead on the row pipeline, as far as it can be seen without a GPU: bin/smcsmc parses -apf_pipeline, the
Python wrapper puts PF_LA_ROW_PIPELINE into pf_lookahead.flags (the field that was `reserved`: same offset, same size), and the oracle,
which has no such path, is always handed 0."""
import ctypes as C
import json
import subprocess

import numpy as np

import cases
from smcsmc_amd import pf, segments as segmod

BASE = ["-Np", "5", "-t", "1", "-r", "1", "1000"]


def _dump(binary, extra):
    r = subprocess.run([binary] + BASE + extra + ["-dumpmodel"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_the_option_table_parses_apf_pipeline(built_binary):
    assert _dump(built_binary, [])["apf_pipeline"] is False
    m = _dump(built_binary, ["-apf", "2", "-apf_pipeline"])
    assert m["apf"] == 2 and m["apf_pipeline"] is True
    # alone it is accepted and means nothing: there is no look-ahead to move
    m = _dump(built_binary, ["-apf_pipeline"])
    assert m["apf"] == 0 and m["apf_pipeline"] is True
    # it takes no value, and a misspelt neighbour is still refused
    r = subprocess.run([built_binary] + BASE + ["-apf_pipelines", "-dumpmodel"], capture_output=True, text=True)
    assert r.returncode != 0
    helptext = subprocess.run([built_binary, "-help"], capture_output=True, text=True)
    assert "-apf_pipeline" in helptext.stdout + helptext.stderr


def _lookahead(n=4):
    model = cases.make_model(n=n, E=4, L=6e4)
    segs = cases.make_segments(model, seed=3, max_seg_len=5000)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a)))
            for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return model, segs, segmod.pack_lookahead(rows, n)


def test_packed_lookahead_carries_the_flag():
    assert pf.LA_ROW_PIPELINE == 1
    # pf_lookahead.flags is where pf_lookahead.reserved was
    assert pf._Lookahead.flags.offset == 12 and pf._Lookahead.flags.size == 4 and pf._Lookahead.n.offset == 16
    _, _, la = _lookahead()
    tbl = (np.ones((4, len(segmod.TBL_QUANTILES))), 1.0)
    assert pf.PackedLookahead(la, 2, tbl, segmod.TBL_QUANTILES, pipeline=True).struct.flags == 1
    assert pf.PackedLookahead(la, 2, tbl, segmod.TBL_QUANTILES, pipeline=False).struct.flags == 0
    assert pf.PackedLookahead(la, 2, tbl, segmod.TBL_QUANTILES).struct.flags == 0
    s = pf.PackedLookahead(la, 3, tbl, segmod.TBL_QUANTILES, pipeline=True).struct
    assert (s.level, s.max_doubletons, s.n_quantiles, s.n) == (3, int(la["max_doubletons"]), len(segmod.TBL_QUANTILES), len(la["n_doubletons"]))
    assert C.sizeof(pf._Lookahead) == 16 + 8 + 11 * C.sizeof(C.c_void_p) + 8


def test_the_oracle_is_handed_no_flag(oracle):
    model, segs, la = _lookahead()
    o = oracle.Oracle(model, 64, seed=3)
    o.init_prior(segs["start"][0])
    si = o.pack_segments(model, segs)
    o.load_lookahead(la, 2, oracle.terminal_branch_quantiles(model, seed=1, n_trees=2000))
    assert o._la.struct.flags == 0
    o.run(si)
    assert np.isfinite(o.logl())
