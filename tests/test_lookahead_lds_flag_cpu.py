"""The switch of the look-ahead on the LDS-tree row pipelines (pf_lookahead.flags bit 2, PF_LA_ROW_PIPELINE_LDS), as far as it shows without
a device: the flag word the python binding packs, the oracle's untouched copy of it, and the option -apf_lds of bin/smcsmc."""
import inspect
import json
import subprocess

import numpy as np

import cases
from smcsmc_amd import ParticleFilter, pf, segments as segmod


def _lookahead(n):
    base = cases.make_model(n=n, E=4, L=4e4)
    segs = cases.make_segments(base, seed=3, max_seg_len=4000)
    rows = [(int(s) + 1, int(l), int(st), list(map(int, a))) for s, l, st, a in zip(segs["start"], segs["length"], segs["state"], segs["alleles"])]
    return base, segs, segmod.pack_lookahead(rows, n)


def test_the_flag_word(oracle):
    assert (pf.LA_ROW_PIPELINE, pf.LA_ROW_PIPELINE_MP, pf.LA_ROW_PIPELINE_LDS) == (1, 2, 4)
    n = 12
    _, _, la = _lookahead(n)
    q = segmod.TBL_QUANTILES
    tbl = (np.arange(n * len(q), dtype=np.float64).reshape(n, len(q)) + 1.0, 123.5)
    plain = pf.PackedLookahead(la, 3, tbl, q)
    lds = pf.PackedLookahead(la, 3, tbl, q, lds=True)
    every = pf.PackedLookahead(la, 3, tbl, q, pipeline=True, structured=True, lds=True)
    assert (plain.struct.flags, lds.struct.flags, every.struct.flags) == (0, 4, 7)
    assert pf.PackedLookahead(la, 3, tbl, q, pipeline=True, lds=True).struct.flags == 5
    for other in (lds, every):
        for name in ("level", "max_doubletons", "n_quantiles", "n", "mean_total_branch_length"):
            assert getattr(other.struct, name) == getattr(plain.struct, name), name
        for a, b in zip(other.a, plain.a):
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    assert (plain.struct.level, plain.struct.n, plain.struct.n_quantiles) == (3, len(la["n_doubletons"]), len(q))
    sig = inspect.signature(ParticleFilter.load_lookahead).parameters
    assert sig["lds"].default is False and sig["pipeline"].default is False and sig["structured"].default is False
    assert inspect.signature(pf.PackedLookahead.__init__).parameters["lds"].default is False
    # the oracle has no such switch: it is handed 0, with and without structure
    base, segs, la = _lookahead(n)
    for model in (base, cases.make_structured(base, P=2, split_epoch=2, mig=1.5)):
        tbl = oracle.terminal_branch_quantiles(model, seed=1, n_trees=200)
        o = oracle.Oracle(model, 16, seed=1)
        o.init_prior(segs["start"][0])
        o.load_lookahead(la, 2, tbl)
        assert o._la.struct.flags == 0 and o._la.struct.level == 2
        o.close()


def test_the_binary_has_the_option(built_binary):
    core = ["-nsam", "12", "-Np", "10", "-t", "10", "-r", "4", "100000", "-apf", "2"]
    r = subprocess.run([built_binary] + core + ["-apf_lds", "-dumpmodel"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout)
    assert m["apf"] == 2 and m["apf_lds"] is True and m["apf_pipeline"] is False and m["mp_rows"] is False
    keys = list(m)
    assert keys.index("apf_lds") == keys.index("mp_rows") + 1
    m = json.loads(subprocess.run([built_binary] + core + ["-apf_pipeline", "-dumpmodel"], capture_output=True, text=True).stdout)
    assert m["apf_lds"] is False and m["apf_pipeline"] is True
    r = subprocess.run([built_binary] + core + ["-apf_ldsx", "-dumpmodel"], capture_output=True, text=True)
    assert r.returncode != 0 and "-apf_ldsx" in r.stderr
    text = subprocess.run([built_binary, "-help"], capture_output=True, text=True)
    text = text.stdout + text.stderr
    line = [ln for ln in text.splitlines() if "-apf_lds " in ln]
    assert len(line) == 1 and "9 to 16" in line[0] and "-mp_rows" in line[0]
