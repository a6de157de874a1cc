"""A numpy model of the lane maps that the wavefront primitives of pf_device.h use instead of __shfl (no GPU).

The sums and scans of a wavefront are part of the canonical arithmetic: wave_tree_sum is the xor butterfly (oracle tree64),
wave_hs_scan the Hillis-Steele scan (oracle hs64), and the association of every addition decides the last bit.  The forms without
LDS keep the operand pairs and change how the operands travel.  This file writes the lane maps down -- quad permutations, the two
mirrors, wave_shr:1, row_shr, row_ror, the two lane swaps -- replays the sequences of pf_device.h on them and compares bits with
the butterfly and the scan.  Inputs spread over hundreds of decades with mixed magnitudes, so that the association matters; the
other associations must differ on them, or the comparison would prove nothing: the serial sum does, and so does the scan that the
row shifts and row broadcasts of wave_total_dpp build in the lanes below 63.  (Its lane 63 does not: the total of those steps is the
balanced tree of the butterfly, operand for operand up to commutation -- asserted below, since it is what one would not expect.)
(What the maps of the hardware are is the business of tests/test_gpu_wave_prims.py.)"""
import numpy as np

LANES = np.arange(64)
ROW = LANES // 16
POS = LANES % 16


# ---- lane maps: src[i] is the lane that lane i reads; -1 = no source, the lane keeps `old`
def quad_perm(p):
    return (LANES // 4) * 4 + np.asarray(p)[LANES % 4]


ROW_HALF_MIRROR = (LANES // 8) * 8 + (7 - LANES % 8)
ROW_MIRROR = ROW * 16 + (15 - POS)
WAVE_SHR1 = LANES - 1                                   # lane 0: -1


def row_shr(d):
    return np.where(POS >= d, LANES - d, -1)


def row_ror(d):
    return ROW * 16 + (POS - d) % 16


def row_bcast15():
    return np.where(ROW >= 1, ROW * 16 - 1, -1)


def row_bcast31():
    return np.where(ROW >= 2, 31, -1)


def dpp(old, src, lane_map, row_mask=0xf):
    ok = (lane_map >= 0) & (((row_mask >> ROW) & 1) == 1)
    return np.where(ok, src[np.maximum(lane_map, 0)], old)


def swap16(a, b):
    """v_permlane16_swap: the odd rows of the first operand change places with the even rows of the second"""
    a, b = a.copy(), b.copy()
    for r in (0, 2):
        lo, hi = slice(16 * r, 16 * r + 16), slice(16 * r + 16, 16 * r + 32)
        a[hi], b[lo] = b[lo].copy(), a[hi].copy()
    return a, b


def swap32(a, b):
    """v_permlane32_swap: the upper half of the first operand changes places with the lower half of the second"""
    a, b = a.copy(), b.copy()
    a[32:], b[:32] = b[:32].copy(), a[32:].copy()
    return a, b


def row_up(v):
    a, b = swap16(v, v)
    h, _ = swap32(b, b)
    return np.where((LANES & 16) != 0, a, h)


# ---- the sequences of pf_device.h
def tree_sum_new(v):
    for m in (quad_perm([1, 0, 3, 2]), quad_perm([2, 3, 0, 1]), ROW_HALF_MIRROR, ROW_MIRROR):
        v = v + dpp(v, v, m)
    a, b = swap16(v, v)
    v = a + b
    a, b = swap32(v, v)
    return a + b


def hs_scan_new(v):
    o = dpp(v, v, WAVE_SHR1)
    v = np.where(LANES >= 1, o + v, v)
    o = dpp(v, v, WAVE_SHR1); o = dpp(o, o, WAVE_SHR1)
    v = np.where(LANES >= 2, o + v, v)
    for d in (4, 8):
        o = dpp(dpp(v, row_up(v), row_ror(d)), v, row_shr(d))
        v = np.where(LANES >= d, o + v, v)
    o = row_up(v)
    v = np.where(LANES >= 16, o + v, v)
    o, _ = swap32(v, v)
    return np.where(LANES >= 32, o + v, v)


def max_scan_new(v):
    for m, rm in ((row_shr(1), 0xf), (row_shr(2), 0xf), (row_shr(4), 0xf), (row_shr(8), 0xf), (row_bcast15(), 0xa), (row_bcast31(), 0xc)):
        o = dpp(v, v, m, rm)
        v = np.where(o > v, o, v)
    return v


def minmax_new(v):
    mn, mx = v.copy(), v.copy()
    for m in (quad_perm([1, 0, 3, 2]), quad_perm([2, 3, 0, 1]), ROW_HALF_MIRROR, ROW_MIRROR):
        mn = np.minimum(mn, dpp(mn, mn, m)); mx = np.maximum(mx, dpp(mx, mx, m))
    for sw in (swap16, swap32):
        a, b = sw(mn, mn); mn = np.minimum(a, b)
        a, b = sw(mx, mx); mx = np.maximum(a, b)
    return mn, mx


# ---- what they have to equal: the canonical forms (__shfl_xor / __shfl_up, oracle tree64 / hs64)
def tree_sum_ref(v):
    for m in (1, 2, 4, 8, 16, 32):
        v = v + v[LANES ^ m]
    return v


def hs_scan_ref(v):
    for d in (1, 2, 4, 8, 16, 32):
        o = v[np.maximum(LANES - d, 0)]
        v = np.where(LANES >= d, o + v, v)
    return v


def max_scan_ref(v):
    for d in (1, 2, 4, 8, 16, 32):
        o = v[np.maximum(LANES - d, 0)]
        v = np.where((LANES >= d) & (o > v), o, v)
    return v


def total_dpp(v):
    """the steps of wave_total_dpp in every lane: row shifts and row broadcasts, a scan whose lane 63 is the total"""
    for m, rm in ((row_shr(1), 0xf), (row_shr(2), 0xf), (row_shr(4), 0xf), (row_shr(8), 0xf), (row_bcast15(), 0xa), (row_bcast31(), 0xc)):
        v = v + dpp(np.zeros(64), v, m, rm)
    return v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _inputs():
    rng = np.random.default_rng(14)
    out = []
    for k in range(400):
        spread = (5.0, 40.0, 150.0, 300.0)[k % 4]              # decades either side of one: up to 600 in all
        out.append(10.0 ** rng.uniform(-spread, spread, 64) * (1.0 + rng.random(64)))
    for k in range(100):                                        # near-equal magnitudes: every addition rounds
        out.append(1.0 + rng.random(64))
    for k in range(64):                                         # one huge value among tiny ones, at every lane
        v = 10.0 ** rng.uniform(-300.0, -280.0, 64); v[k] = 1e300 * (1.0 + rng.random())
        out.append(v)
    z = np.zeros(64); z[::3] = -0.0; z[5] = 5e-324; z[40] = -5e-324
    out.append(z)
    out.append(np.full(64, -0.0))
    return out


def test_lane_maps_are_what_the_sequences_assume():
    ident = LANES.astype(np.float64)
    # after the step with mask m the 2m lanes of a group hold equal bits, and each map reads a lane of the partner group
    for m, lane_map in ((1, quad_perm([1, 0, 3, 2])), (2, quad_perm([2, 3, 0, 1])), (4, ROW_HALF_MIRROR), (8, ROW_MIRROR)):
        assert ((lane_map // m) == ((LANES ^ m) // m)).all(), m
    a, b = swap16(ident, ident)
    assert (a // 16 == [0] * 16 + [0] * 16 + [2] * 16 + [2] * 16).all() and (b // 16 == [1] * 16 + [1] * 16 + [3] * 16 + [3] * 16).all()
    assert (a % 16 == POS).all() and (b % 16 == POS).all()
    a, b = swap32(ident, ident)
    assert (a == LANES % 32).all() and (b == 32 + LANES % 32).all()
    assert (row_up(ident)[16:] == LANES[16:] - 16).all()
    for d in (4, 8):
        o = dpp(dpp(ident, row_up(ident), row_ror(d)), ident, row_shr(d))
        assert (o[d:] == LANES[d:] - d).all(), d
    o = dpp(ident, ident, WAVE_SHR1)
    assert o[0] == 0 and (o[1:] == LANES[1:] - 1).all()


def test_new_sequences_give_the_bits_of_the_butterfly_and_of_the_scan():
    differs_sum = differs_scan = differs_rows = 0
    for v in _inputs():
        for x in (v, np.where(LANES % 5 == 0, -v, v)):          # mixed signs for the sums
            ref = tree_sum_ref(x)
            assert (_bits(ref) == _bits(ref[0])).all()           # every lane the same total
            assert (_bits(tree_sum_new(x)) == _bits(ref)).all()
            serial = 0.0
            for t in x:
                serial = serial + t
            differs_sum += int(_bits([serial])[0] != _bits(ref)[0])
            assert _bits(total_dpp(x))[63] == _bits(ref)[63]      # the row-shift total is the same tree as the butterfly
        ref = hs_scan_ref(v)
        assert (_bits(hs_scan_new(v)) == _bits(ref)).all()
        differs_scan += int((_bits(np.cumsum(v)) != _bits(ref)).any())
        differs_rows += int((_bits(total_dpp(v)) != _bits(ref)).any())
        assert (_bits(max_scan_new(v)) == _bits(max_scan_ref(v))).all()
        s = np.where(LANES % 7 == 0, -ref, ref)                  # a scan that is not monotone
        assert (_bits(max_scan_new(s)) == _bits(max_scan_ref(s))).all()
    # the inputs do tell associations apart: the serial sum, the serial scan and the row-shift scan give other bits on many of them
    assert differs_sum > 100, differs_sum
    assert differs_scan > 100, differs_scan
    assert differs_rows > 100, differs_rows


def test_zeros_of_both_signs_keep_their_sign():
    z = np.zeros(64); z[::2] = -0.0
    for v in (z, -z, np.full(64, -0.0), np.where(LANES < 20, -0.0, 0.0), np.where(LANES < 20, 0.0, -0.0)):
        assert (_bits(hs_scan_new(v)) == _bits(hs_scan_ref(v))).all()
        assert (_bits(max_scan_new(v)) == _bits(max_scan_ref(v))).all()
        assert (_bits(tree_sum_new(v)) == _bits(tree_sum_ref(v))).all()


def test_integer_forms():
    rng = np.random.default_rng(5)
    i32 = np.iinfo(np.int32)
    for k in range(200):
        v = rng.integers(-5, 5, 64) if k % 2 else rng.integers(i32.min, i32.max, 64, endpoint=True)
        if k % 10 == 0:
            v[rng.integers(64)] = i32.min; v[rng.integers(64)] = i32.max
        mn, mx = minmax_new(v)
        assert (mn == v.min()).all() and (mx == v.max()).all()
        assert (max_scan_new(v) == np.maximum.accumulate(v)).all()
