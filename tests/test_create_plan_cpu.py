"""The first two steps of pf_create on a machine without a device (pf_test_plan): every refusal that needs no device, with the texts of
the commit before the creation was split into steps, and the plan of a handle -- the rings tests/test_gpu_run_path.py's table implies for
each of its rows, and the fields the allocation follows.  Not covered: the refusals that need a device (no device, device index, streams,
events, the LDS limits of step four).  And a look at the sources: one owner of device memory, one place that deletes a handle."""
import math
import os
import re

import numpy as np
import pytest

import cases
from smcsmc_amd import pf
from test_gpu_run_path import E, FORCE_WIDE, K_PIPE, NP, PF_RING, TABLE, _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smcsmc_amd", "csrc")
NO_DRAW_TABLE = 128


@pytest.fixture(scope="module", autouse=True)
def lib():
    from smcsmc_amd import build
    build.build_lib()
    return pf.load_library()


def _plan(n=4, P=1, kind="plain", Np=NP, apf=False, tweak=None, model=None, **kw):
    return pf.plan(_inputs(n, P, kind)[1] if model is None else model, Np, tweak=tweak, seed=5, **kw)


# ---------------------------------------------------------------- refusals
def _set(**fields):
    """tweak: fields of pf_model (m_*) or pf_params (p_*) set after packing, past what the Python side would pass on"""
    def tweak(m, p):
        for k, v in fields.items():
            setattr(m if k.startswith("m_") else p, k[2:], v)
    return tweak


def _guide(positions, rates, leaf=1.0, n=4):
    K = len(positions)
    return dict(positions=np.asarray(positions, float), rates=np.asarray(rates, float), leaf_rates=np.full((K, n), leaf))


def _guided(**g):
    base = _inputs(4)[0]
    return dict(base, guide=_guide(**g), application_delays=np.full(E, 3000.0))


REMOVED = {64: "one population as two launches on two streams", 512: "count workgroups in ascending epoch order",
           1024: "the two streams on disjoint compute units", 8192: "hand-off between launches through counters in memory"}

REFUSALS = [(dict(debug=bit), "pf_create: pf_params.debug bit %d (%s) selected a launch arrangement that has been removed" % (bit, what))
            for bit, what in REMOVED.items()] + [
    (dict(log_cap=-1), "pf_create: ring capacities out of range"),
    (dict(piece_cap=1 << 31), "pf_create: ring capacities out of range"),
    (dict(gen_cap=3), "pf_create: log_cap and gen_cap must be at least 4"),
    (dict(log_cap=2), "pf_create: log_cap and gen_cap must be at least 4"),
    (dict(P=2, gen_cap=PF_RING + 3), "pf_create: gen_cap must be at least 20 when the extend role runs ahead of the counts (structured models)"),
    (dict(tweak=_set(m_n_pops=5)), "pf_create: n_pops must be in 1..4"),
    (dict(tweak=_set(m_n_pops=0)), "pf_create: n_pops must be in 1..4"),
    (dict(tweak=_set(m_nsam=65)), "pf_create: nsam must be in 2..64"),
    (dict(tweak=_set(m_nsam=1)), "pf_create: nsam must be in 2..64"),
    (dict(P=2, tweak=_set(m_nsam=17)), "pf_create: more than 16 haplotypes need one population (structured models take nsam <= 16)"),
    (dict(P=2, debug=FORCE_WIDE), "pf_create: PF_DEBUG_FORCE_WIDE applies to one population only"),
    (dict(n=17, record_trees=True), "pf_create: tree recording (-arg) needs nsam <= 16 (its descendant masks are 32 bits wide)"),
    (dict(n=5, debug=FORCE_WIDE, record_trees=True), "pf_create: tree recording (-arg) needs nsam <= 16 (its descendant masks are 32 bits wide)"),
    (dict(tweak=_set(m_n_epochs=65)), "pf_create: n_epochs must be in 1..64"),
    (dict(tweak=_set(m_n_epochs=0)), "pf_create: n_epochs must be in 1..64"),
    (dict(Np=0), "pf_create: np must be in 1..262144"),
    (dict(Np=262145), "pf_create: np must be in 1..262144"),
    (dict(tweak=_set(m_n_bias_heights=9)), "pf_create: at most 8 bias heights are supported"),
    (dict(tweak=_set(m_n_bias_heights=1)), "pf_create: bias_heights, bias_strengths and application_delays must all be given"),
    (dict(tweak=_set(m_n_rate_segments=1)), "pf_create: rate_positions, rate_values, leaf_rel_rates and application_delays must all be given with a guide"),
    (dict(model=_guided(positions=[5.0, 100.0], rates=[1e-8, 2e-8])), "pf_create: the recombination guide must start at position 0"),
    (dict(model=_guided(positions=[0.0, 100.0, 100.0], rates=[1e-8, 2e-8, 1e-8])), "pf_create: guide segment starts must increase"),
    (dict(model=_guided(positions=[0.0, 100.0], rates=[1e-8, 0.0])), "pf_create: guide recombination rates must be positive"),
    (dict(model=_guided(positions=[0.0, 100.0], rates=[1e-8, 2e-8], leaf=0.0)), "pf_create: relative leaf rates of the guide must be positive"),
    (dict(P=2, mig_cap=4097), "pf_create: mig_cap out of range"),
    (dict(model=dict(_inputs(4)[0], vb_coal_counts=[3.0, 0.0, 2.0, 1.0])), "pf_create: variational-Bayes event counts must be positive"),
    (dict(model=dict(_inputs(4)[0], vb_coal_counts=[3.0, 1.0, 2.0, -1.0])), "pf_create: variational-Bayes event counts must be positive"),
    (dict(model=dict(_inputs(4, 2)[1], vb_coal_counts=np.ones(E * 2), vb_mig_counts=np.r_[np.ones(E * 4 - 1), 0.0])),
     "pf_create: variational-Bayes event counts must be positive"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=["%02d-%s" % (i, r[1][11:40].replace(" ", "-")) for i, r in enumerate(REFUSALS)])
def test_a_refusal_that_needs_no_device(kw, text):
    with pytest.raises(pf.PfError) as e:
        _plan(**kw)
    assert str(e.value) == text


def test_null_model_or_parameters_are_refused(lib):
    assert lib.pf_test_plan(None, None, None, 0) == -1
    assert lib.pf_last_error().decode() == "pf_create: null model or parameters"


def test_refusals_keep_their_order():
    """a removed debug bit before a bad np; a ring capacity before the model's shape; the model's shape before mig_cap and the event counts"""
    with pytest.raises(pf.PfError, match="has been removed"):
        _plan(Np=0, debug=64)
    with pytest.raises(pf.PfError, match="ring capacities out of range"):
        _plan(log_cap=-1, tweak=_set(m_nsam=65))
    with pytest.raises(pf.PfError, match="nsam must be in 2..64"):
        _plan(P=2, mig_cap=5000, tweak=_set(m_nsam=65))
    with pytest.raises(pf.PfError, match="mig_cap out of range"):
        _plan(mig_cap=5000, model=dict(_inputs(4, 2)[1], vb_coal_counts=np.zeros(E * 2)))


def test_a_small_output_buffer_is_refused(lib):
    f = pf.ParticleFilter.__new__(pf.ParticleFilter)
    f.h = None
    f._pack(_inputs(4)[1], NP)
    out = np.zeros(16 + E, np.int32)
    import ctypes as C
    assert lib.pf_test_plan(C.byref(f._model), C.byref(f._params), out.ctypes.data, len(out)) == -1
    assert lib.pf_test_plan(C.byref(f._model), C.byref(f._params), np.zeros(16 + E + 1, np.int32).ctypes.data, 16 + E + 1) == 16 + E + 1


# ---------------------------------------------------------------- the plan
def _key(kw):
    return tuple(sorted((k, v) for k, v in kw.items() if k != "apf"))


def _rings_of_row(kw, one, many):
    if "SweepXmp" in (one, many):
        return "Xmp"
    if "SweepXl" in (one, many):
        return "Xl"
    if kw.get("P", 1) == 1 and kw["n"] <= 8 and kw.get("Np", NP) <= 131072 and not kw.get("debug", 0) & FORCE_WIDE:
        return "Reg"     # (there also where a switch takes the rows elsewhere: allocated, unused)
    return None


# a look-ahead is loaded into a handle that exists: the plan of such a row is that of the same handle without one
WITHOUT_LOOKAHEAD = {_key(kw): _rings_of_row(kw, one, many) for _, kw, one, many in TABLE if not kw.get("apf")}


@pytest.mark.parametrize("kw,one,many", [pytest.param(*row[1:], id=row[0]) for row in TABLE])
def test_rings_of_every_row_of_the_run_path_table(kw, one, many):
    want = WITHOUT_LOOKAHEAD[_key(kw)] if kw.get("apf") else _rings_of_row(kw, one, many)
    pl = _plan(**kw)
    assert pl["rings"] == want
    assert pl["nslots"] == (16 if want else 2)
    assert (pl["smem_pipe"] > 0) == (want is not None)
    assert pl["draw_table"] == (want == "Reg" and not kw.get("debug", 0) & (K_PIPE | NO_DRAW_TABLE))
    focused = kw.get("kind", "plain") != "plain"
    assert pl["workers"] == 0          # nobody asked for count workers
    asked = _plan(count_workers=7, **kw)["workers"]
    assert asked == (7 if (want == "Reg" and kw["n"] <= 4 and not focused and not kw.get("record_trees") and not kw.get("debug", 0) & K_PIPE) else 0)


def test_the_table_has_its_39_rows_and_the_cases_the_plan_is_about():
    assert len(TABLE) == 39
    ids = [r[0] for r in TABLE]
    for must in ("n2-131073-particles", "n9-short-generation-ring", "n9-generation-ring", "n17", "n5-force-wide", "P2-n8-arg", "n16-arg"):
        assert must in ids


def test_rings_at_the_particle_threshold():
    assert _plan(n=2, Np=131072, gen_cap=32, log_cap=32)["rings"] == "Reg"
    assert _plan(n=2, Np=131073, gen_cap=32, log_cap=32)["rings"] is None
    assert _plan(n=9, gen_cap=PF_RING + 3)["rings"] is None
    assert _plan(n=9, gen_cap=PF_RING + 4)["rings"] == "Xl"


def test_no_draw_table_switch():
    assert _plan(n=4)["draw_table"] is True
    assert _plan(n=4, debug=NO_DRAW_TABLE)["draw_table"] is False
    assert _plan(n=4, debug=K_PIPE)["draw_table"] is False


def test_ledger_workgroups_and_count_columns():
    Np = 4096                                   # sixteen particle blocks of 256
    nblocks = Np // 256
    pl = _plan(n=4, Np=Np)
    assert pl["ledger_wgs"] == 192 and pl["ncw"] == nblocks
    assert pl["cw_off"] == [j * nblocks for j in range(E + 1)]           # count_wgs = 0: every column ncw wide
    lags = [1000.0, 5000.0, 40000.0, 2500.0]
    model = dict(_inputs(4)[0], lags=np.array(lags))
    pl = _plan(model=model, Np=Np, count_wgs=8)
    assert pl["ledger_wgs"] == 32 and pl["ncw"] == 8
    ncw, off = 8, [0]
    for j in range(E):                          # columns oldest epoch first
        lag = lags[E - 1 - j]
        w = math.ceil(ncw * min(1.0, 2500.0 / max(lag, 1.0)))
        off.append(off[-1] + max(min(2, ncw), min(w, ncw)))
    assert pl["cw_off"] == off and off == [0, 8, 10, 14, 22]
    # fewer particle blocks than the caller's count_wgs: a column gets no more than there are
    assert _plan(n=4, Np=512, count_wgs=8)["ncw"] == 2


def test_the_other_fields_of_the_plan():
    pl = _plan(n=4)
    assert (pl["E"], pl["RS"], pl["ncol"], pl["mcap"], pl["dcap"], pl["pcap"], pl["max_trace_events"]) == (E, 8, 6, 96, 128, 0, 64)
    pl = _plan(n=5, debug=FORCE_WIDE)
    assert pl["RS"] == 10                       # the wide kernels' records carry one more word
    pl = _plan(n=4, P=2, mig_cap=40, log_cap=64, gen_cap=64)
    assert (pl["ncol"], pl["mcap"], pl["pcap"]) == (3 * 2 + 3 + 4 + 4, 40, 256)
    assert _plan(n=4, P=3)["ncol"] == 3 * 4 + 3 + 16 + 8     # three populations count on the kernel of four
    assert _plan(n=4, record_trees=True, gen_cap=80, log_cap=64)["max_trace_events"] == 80     # -arg keeps every parent table
    assert _plan(n=4, delay_cap=7, piece_cap=9)["dcap"] == 7
    assert _plan(n=4, debug=5 << 16)["split_batch"] == 5


# ---------------------------------------------------------------- the sources
HOST = ["pf_hip.hip", "pf_run.h", "pf_devmem.h", "pf_handle.h", "pf_create.h", "pf_get.h", "pf_tools.h"]


def test_one_owner_of_device_memory_and_one_place_that_deletes_a_handle():
    text = {f: open(os.path.join(CSRC, f)).read() for f in HOST}
    included = set(re.findall(r'#include "(pf_[a-z_]+\.h)"', text["pf_hip.hip"][text["pf_hip.hip"].index("host side"):]))
    assert included == set(HOST[1:])
    for call in ("hipMalloc(", "hipFree("):
        assert [f for f in HOST if call in text[f]] == ["pf_devmem.h"], call
    deletes = [(f, ln.strip()) for f in HOST for ln in text[f].splitlines() if re.search(r"\bdelete h\b", ln)]
    assert deletes == [("pf_create.h", "void pf_destroy(pf_handle* h) { delete h; }")]
