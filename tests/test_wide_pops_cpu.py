"""Structured models of five to eight populations, without a device: what pf_create decides for them (pf.plan -> pf_test_plan), what the
binary reads from a six-population command line, and the kernels the built library carries for them."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cases
from smcsmc_amd import pf
from smcsmc_amd.pf import PfError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCE_LDS, NO_FUSE = 1, 2


@pytest.fixture(scope="module", autouse=True)
def lib():
    from smcsmc_amd import build
    build.build_lib()
    return pf.load_library()


def _model(n, P, E=8):
    return cases.make_structured(cases.make_model(n=n, E=E, L=1e5), P=P, split_epoch=max(E - 3, 1), mig=2.0)


@pytest.mark.parametrize("kw", [dict(), dict(mp_rows=True), dict(debug=FORCE_LDS), dict(debug=NO_FUSE), dict(record_trees=True, gen_cap=64, log_cap=64)],
                         ids=["plain", "mp-rows", "force-lds", "no-fuse", "arg"])
@pytest.mark.parametrize("n", [2, 8, 9, 16])
@pytest.mark.parametrize("P", [5, 6, 7, 8])
def test_five_to_eight_populations_get_no_rings_and_the_wide_count_columns(P, n, kw):
    pl = pf.plan(_model(n, P), 256, seed=5, **kw)
    assert pl["rings"] is None and pl["nslots"] == 2 and pl["smem_pipe"] == 0 and not pl["draw_table"] and pl["workers"] == 0
    assert pl["ncol"] == 3 * 8 + 3 + 8 * 8 + 2 * 8 == 107          # the columns of AccT<8>, whatever P in 5..8
    assert pl["pcap"] > 0 and pl["mcap"] == 96


def test_up_to_four_populations_keep_their_plan():
    assert [pf.plan(_model(8, P), 256, seed=5)["ncol"] for P in (2, 3, 4)] == [17, 39, 39]
    assert pf.plan(_model(8, 4), 256, seed=5)["rings"] == "Xmp"
    assert pf.plan(_model(8, 4, E=64), 256, seed=5)["E"] == 64             # sixty-four epochs as before


def test_nine_populations_are_refused():
    with pytest.raises(PfError, match=r"n_pops must be in 1\.\.8"):
        pf.plan(_model(8, 9), 256, seed=5)


@pytest.mark.parametrize("P", [5, 8])
def test_without_the_model_bit_nothing_changed(P):
    """PF_MODEL_WIDE_POPS (pf_model.flags bit 2) is what opens five to eight populations; the binding sets it for such a model.  A caller
    that does not gets the refusal it always got, and the bit means nothing up to four populations."""
    def clear(m, p):
        assert m.flags & pf.MODEL_WIDE_POPS
        m.flags &= ~pf.MODEL_WIDE_POPS
    with pytest.raises(PfError) as e:
        pf.plan(_model(8, P), 256, seed=5, tweak=clear)
    assert str(e.value) == "pf_create: n_pops must be in 1..4"

    def set_bit(m, p):
        assert not m.flags & pf.MODEL_WIDE_POPS
        m.flags |= pf.MODEL_WIDE_POPS
    assert pf.plan(_model(8, 4), 256, seed=5, tweak=set_bit) == pf.plan(_model(8, 4), 256, seed=5)


@pytest.mark.parametrize("P", [5, 8])
def test_more_than_32_epochs_are_refused_beyond_four_populations(P):
    assert pf.plan(_model(8, P, E=32), 256, seed=5)["E"] == 32
    with pytest.raises(PfError, match="more than four populations takes at most 32 epochs"):
        pf.plan(_model(8, P, E=33), 256, seed=5)


def test_seventeen_haplotypes_with_structure_are_still_refused():
    with pytest.raises(PfError, match="more than 16 haplotypes need one population"):
        pf.plan(_model(17, 5), 256, seed=5)


def test_the_largest_model_fits_the_lds_and_a_longer_event_list_is_refused_by_the_plan_size():
    """32 epochs, 8 populations, 16 haplotypes: 16 KB of migration rates among the tables, within the 160 KB of a workgroup"""
    assert pf.plan(_model(16, 8, E=32), 256, seed=5)["smem"] <= 160 * 1024
    assert pf.plan(_model(16, 8, E=32), 256, seed=5, mig_cap=600)["smem"] > 160 * 1024      # what pf_create answers "does not fit the LDS" to


def test_binary_reads_six_populations():
    binary = os.path.join(ROOT, "bin", "smcsmc")
    L = 200000
    core = ("-N0 10000 -t %g -r %g %d -I 6 1 1 1 1 1 1 -eN 0.0 1.0 -eM 0.0 5.0 -en 0.1 6 0.5 -ema 0.1" % (4e4 * 2.5e-8 * L, 4e4 * 1e-8 * L, L)).split()
    rows = [[0 if a == b else (a + 1) * 0.1 + b * 0.01 for b in range(6)] for a in range(6)]
    core += ["%g" % v for row in rows for v in row]
    core += ["-em", "0.2", "6", "1", "3.0", "-eN", "0.5", "1.0", "-eM", "0.5", "0"]
    for k in range(2, 7):
        core += ["-ej", "0.5", str(k), "1"]
    r = subprocess.run([binary] + core + ["-nsam", "6", "-tmax", "4", "-dumpmodel"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout)
    E = len(m["change_times"])
    assert m["npop"] == 6 and m["sample_pops"] == [0, 1, 2, 3, 4, 5] and E == 4
    mig = np.array(m["mig_rates"]).reshape(E, 6, 6); smig = np.array(m["single_mig"]).reshape(E, 6, 6)
    ps = np.array(m["pop_sizes"]).reshape(E, 6)
    N0 = m["N0"]
    assert np.allclose(mig[0][~np.eye(6, dtype=bool)], 1.0 / (4 * N0)) and (np.diag(mig[0]) == 0).all()      # -eM 5: 5 / (P - 1) per pair
    assert np.allclose(mig[1] * 4 * N0, rows)                                                                   # -ema: the whole matrix
    assert mig[2, 5, 0] == pytest.approx(3.0 / (4 * N0)) and mig[2, 4, 0] == pytest.approx(rows[4][0] / (4 * N0))   # -em on one pair
    assert ps[1, 5] == pytest.approx(0.5 * N0) and ps[1, 4] == pytest.approx(N0) and ps[3, 5] == pytest.approx(N0)   # -en on population 6
    assert mig[3].sum() == 0 and (smig[3, 1:, 0] == 1.0).all() and smig[:3].sum() == 0                           # -ej: everybody joins population 1


def _all_kernels(lib_path):
    """kernel_meta.kernels() of every offload bundle of the library (it reads the first one of the file it is given: pf_hip's)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import kernel_meta
    b = open(lib_path, "rb").read()
    out = {}
    i = b.find(b"__CLANG_OFFLOAD_BUNDLE__")
    while i >= 0:
        with tempfile.NamedTemporaryFile(suffix=".bundle") as t:
            t.write(b[i:]); t.flush()
            out.update(kernel_meta.kernels(t.name))
        i = b.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 1)
    return out


def test_the_library_carries_the_wide_instances_without_scratch():
    from smcsmc_amd import build
    meta = _all_kernels(build.build_lib())
    # k_count<8, 8>, k_count<16, 8>: per-population statistics in registers, the migration counts in LDS -- no scratch, and no more than the
    # 256 architectural registers a wavefront has without AGPR spills
    for k in ("_Z7k_countILi8ELi8EEv5KArgsi7Windows", "_Z7k_countILi16ELi8EEv5KArgsi7Windows"):
        assert k in meta, sorted(x for x in meta if "k_count" in x)
        assert meta[k]["scratch"] == 0 and meta[k]["vgpr"] <= 256 and meta[k]["agpr"] == 0, (k, meta[k])
    # k_extend_mp<BIASED, TREES, 8>: the eight counters of the wide walk stay in registers
    for biased in (0, 1):
        for trees in (0, 1):
            k = "_Z11k_extend_mpILb%dELb%dELi8EEv5KArgsx" % (biased, trees)
            assert k in meta, sorted(x for x in meta if "k_extend_mp" in x)
            assert meta[k]["scratch"] == 0, (k, meta[k])
            narrow = meta["_Z11k_extend_mpILb%dELb%dELi4EEv5KArgsx" % (biased, trees)]
            assert narrow["scratch"] == 0 and meta[k]["vgpr"] + meta[k]["agpr"] <= narrow["vgpr"] + narrow["agpr"] + 16, (k, meta[k], narrow)
    for k in ("_Z9k_init_mpILi8EEv5KArgsd", "_Z14k_calibrate_mpILi8EEv5KArgsyxxPiPdS1_", "_Z8k_tbl_mpILi8EEv5KArgsyxPdS1_Pi"):
        assert k in meta and meta[k]["scratch"] == 0, (k, meta.get(k))
