"""The plan of a handle created with pf_params.flags bit 3 (PF_FLAG_MP_LDS_ROWS, ParticleFilter(..., mp_rows=True)), without a device
(pf.plan -> pf_test_plan): the rings of the row pipeline for a structured model of 9 to 16 haplotypes that qualifies, and for every
other handle exactly what it gets without the flag -- the same plan field for field, or the same refusal."""
import pytest

from smcsmc_amd import pf
from smcsmc_amd.pf import PfError
from test_gpu_run_path import FORCE_LDS, K_PIPE, NO_FUSE, NP, PF_RING, TABLE, TWO_LAUNCH, _inputs


@pytest.fixture(scope="module", autouse=True)
def lib():
    from smcsmc_amd import build
    build.build_lib()
    return pf.load_library()


def _plan(n=4, P=1, kind="plain", Np=NP, apf=False, **kw):
    return pf.plan(_inputs(n, P, kind)[1], Np, seed=5, **kw)


def _outcome(**kw):
    """the plan, or the text of the refusal"""
    try:
        return _plan(**kw)
    except PfError as e:
        return str(e)


@pytest.mark.parametrize("P", [2, 3, 4])
@pytest.mark.parametrize("n", [9, 16])
@pytest.mark.parametrize("kind", ["plain", "focused"])
def test_the_flag_gives_the_rings_of_the_row_pipeline(P, n, kind):
    pl = _plan(n=n, P=P, kind=kind, mp_rows=True)
    assert pl["rings"] == "Xlmp" and pl["nslots"] == 16 and pl["smem_pipe"] > 0
    assert not pl["draw_table"] and pl["workers"] == 0
    off = _plan(n=n, P=P, kind=kind)
    assert off["rings"] is None and off["nslots"] == 2 and off["smem_pipe"] == 0
    # nothing else of the plan depends on the flag
    for k in pl:
        if k not in ("rings", "nslots", "smem_pipe"):
            assert pl[k] == off[k], k


def test_the_names_grow_at_the_end():
    assert pf.RINGS == (None, "Reg", "Xmp", "Xl", "Xlmp")
    assert pf.RUN_PATHS == ("General", "TwoLaunch", "KPipe", "Sweep", "SweepSplit", "SweepXmp", "SweepXl", "SweepXlmp")


NOT_QUALIFYING = [
    ("n8", dict(n=8, P=2), "Xmp"),
    ("P1-n12", dict(n=12), "Xl"),
    ("record-trees", dict(n=12, P=2, record_trees=True, gen_cap=64, log_cap=64), None),
    ("131073-particles", dict(n=9, P=2, Np=131073, gen_cap=32, log_cap=32), None),
    ("force-lds", dict(n=12, P=2, debug=FORCE_LDS), None),
    ("no-fuse", dict(n=12, P=2, debug=NO_FUSE), None),
    ("k-pipe", dict(n=12, P=2, debug=K_PIPE), None),
    ("two-launch", dict(n=12, P=2, debug=TWO_LAUNCH), None),
]


@pytest.mark.parametrize("kw,rings", [pytest.param(*r[1:], id=r[0]) for r in NOT_QUALIFYING])
def test_a_handle_that_does_not_qualify_keeps_its_plan(kw, rings):
    without = _plan(**kw)
    assert without["rings"] == rings
    assert _plan(mp_rows=True, **kw) == without


def test_at_the_particle_threshold_and_the_generation_ring():
    assert _plan(n=9, P=2, Np=131072, gen_cap=32, log_cap=32, mp_rows=True)["rings"] == "Xlmp"
    assert _plan(n=9, P=2, gen_cap=PF_RING + 4, mp_rows=True)["rings"] == "Xlmp"
    # a generation ring of PF_RING + 3 is refused for every structured model, whatever the flag says
    short = _outcome(n=9, P=2, gen_cap=PF_RING + 3)
    assert isinstance(short, str) and "gen_cap must be at least 20" in short
    assert _outcome(n=9, P=2, gen_cap=PF_RING + 3, mp_rows=True) == short


def test_a_small_mig_cap_puts_the_decision_tables_behind_the_state():
    """mig_cap = 8: 512 doubles of migration times a workgroup, fewer than the tables of the prologue take -- they go behind the state,
    which still fits; the plan (its LDS is that of the general kernels) says Xlmp either way"""
    assert _plan(n=16, P=4, mig_cap=8, mp_rows=True)["rings"] == "Xlmp"
    assert _plan(n=16, P=4, mig_cap=8, Np=131072, gen_cap=32, log_cap=32, mp_rows=True)["rings"] == "Xlmp"


@pytest.mark.parametrize("kw,one,many", [pytest.param(*row[1:], id=row[0]) for row in TABLE])
def test_the_rows_of_the_run_path_table_with_the_flag(kw, one, many):
    without = _outcome(**kw)
    flagged = _outcome(mp_rows=True, **kw)
    if kw.get("P", 1) > 1 and kw["n"] > 8:
        assert kw == dict(n=9, P=2)                      # the one row of the table the flag has a meaning for
        assert without["rings"] is None and flagged["rings"] == "Xlmp"
    else:
        assert flagged == without
