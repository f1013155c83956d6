"""The long double reference of the fused synthesis pass (tests/synth_reference.py) and its derived bound, on the CPU: an honest fp64
evaluation of the same formula stays inside the bound at every element of every case the GPU test runs (tests/synth_cases.py), and
each of twelve deliberately wrong evaluations - one per place where a kernel of this shape can go wrong - leaves it by a factor of
at least 1e6 at some element of every case that exercises the mutated path.  The factor is a condition on the cases' operands, not a
tolerance: they are O(1), so a wrong term is O(1) against a bound near 1e-14.

The evaluation below walks the tile table the way a kernel does (tile by tile, rows of a padded NaN buffer) so that the mutants can be
said in a kernel's terms; the reference it is held against does not."""
import numpy as np
import pytest

import synth_cases as sc
from oracle import philox_ref
from synth_reference import HAVE_LONG_DOUBLE, deviate_pairs, synth_reference, wn_pair_and_branch

pytestmark = pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")

PAD_ROWS, PAD_LEFT, PAD_COLS = 1, 3, 6


def evaluate(case, mutant=None):
    """fp64 NumPy evaluation with libm deviates into the view [R, n_toa] at column PAD_LEFT of a NaN-filled [R + 1, n_toa + 6] buffer
    (returned whole)."""
    pa, seed, r0, R, single = case["pa"], case["seed"], case["r0"], case["R"], case["single"]
    mode = "fast" if case["fast"] else "f64"
    n, P, K = pa["n_toa"], pa["n_psr"], pa["rn_k"]
    big = np.full((R + PAD_ROWS, n + PAD_COLS), np.nan)
    out = big[:R, PAD_LEFT:PAD_LEFT + n]
    after = []
    ntl = len(pa["tile_psr"])
    for t in range(ntl):
        a, s, c = int(pa["tile_psr"][t]), int(pa["tile_start"][t]), int(pa["tile_count"][t])
        sl = slice(s, s + c)
        a_rng = int(pa["tile_psr"][t - 1]) if mutant == "stream_psr_of_previous_tile" else a
        v = np.zeros((R, c))
        if K:
            F, cf = pa["Ft"][:, sl], pa["rn_coef"][:R, a, :]
            if mutant == "last_bin_dropped":
                v += cf[:, :K - 1] @ F[:K - 1]
            elif mutant == "bins_from_12_swapped":
                k = np.arange(K)
                k[12:] ^= 1
                v += cf[:, k] @ F
            else:
                v += cf @ F
            if mutant == "last_group_unclamped":   # bins K .. 4 ceil(K / 4) - 1: whatever lies behind the coefficient and the row
                flat = pa["rn_coef"].reshape(-1)
                for k in range(K, -(-K // 4) * 4):
                    ck = np.take(flat, (np.arange(R) * P + a) * K + k, mode="wrap")
                    v += ck[:, None] * pa["Ft_beyond"][k - K, sl][None, :]
        if pa["gw_npts"]:
            j, G = pa["gw_jlo"][sl].astype(np.int64), pa["gw_G"][:R, a, :]
            g0, g1 = G[:, j], G[:, j if mutant == "bracket_j_for_j_plus_1" else j + 1]
            v += (g1 - g0) * pa["gw_w"][sl] + g0
        for r in range(R):
            real = r0 + r
            if mutant == "row_R_counter_into_row_R_minus_1" and r == R - 1 and R % 16:
                real = r0 + R      # a row beyond R of the group of sixteen, stored last to row R - 1
            if mutant == "high_word_of_realisation_dropped":
                real &= 0xFFFFFFFF
            if pa.get("wn_a") is not None:
                z1, z2 = deviate_pairs(seed, real, philox_ref.stream_id(philox_ref.STREAM_WN, a_rng), pa["idx_in_psr"][sl], mode)
                if mutant == "wn_z1_z2_swapped":
                    z1, z2 = z2, z1
                v[r] += pa["wn_a"][sl] * z1 + pa["wn_b"][sl] * z2
            if pa.get("wn_c") is not None:
                pair, br = wn_pair_and_branch(pa["idx_in_psr"][sl])
                z0, z1 = deviate_pairs(seed, real, philox_ref.stream_id(philox_ref.STREAM_WN, a_rng), pair, mode)
                v[r] += pa["wn_c"][sl] * np.where(br == 1, z1, z0)
            if pa.get("ecorr_toa") is not None:
                e = pa["epoch_of"][sl].astype(np.int64)
                if mutant == "ecorr_one_epoch_on":
                    e = e + 1
                if mutant == "ecorr_branch_swapped":
                    e = e ^ 1
                if mutant == "ecorr_ep0_off_by_one" and pa["tile_epn"][t] > 0:   # staged: offset e - 2 (ep0 + 1) into the tile's deviates
                    e = e - 2
                z0, z1 = deviate_pairs(seed, real, philox_ref.stream_id(philox_ref.STREAM_ECORR, a_rng), e >> 1, mode)
                v[r] += pa["ecorr_toa"][sl] * np.where((e & 1) == 1, z1, z0)
        if pa.get("det") is not None:
            v += pa["det"][sl]
        out[:, sl] = v
        if mutant == "clamped_lane_written_to_count" and c < sc.TILE:
            after.append((s + c, v[:, c - 1].copy()))
    for col, val in after:       # (whichever of two stores to one address lands last: here the wrong one)
        big[:R, PAD_LEFT + col] = val
    return big


def excess(big, ref, bound):
    """max |got - ref| / bound over the view; inf where a value is missing, or present where none belongs (outside the view, or at a
    TOA in no tile)"""
    R, n = ref.shape
    view = big[:R, PAD_LEFT:PAD_LEFT + n]
    outside = big.copy()
    outside[:R, PAD_LEFT:PAD_LEFT + n] = np.nan
    hole = np.isnan(ref)
    if not np.all(np.isnan(outside)) or not np.all(np.isnan(view[hole])) or not np.all(np.isfinite(view[~hole])):
        return np.inf
    err = np.abs(view[~hole].astype(np.longdouble) - ref[~hole]).astype(np.float64)
    b = bound[~hole]
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def _draws(case):
    pa = case["pa"]
    return pa.get("wn_a") is not None or pa.get("wn_c") is not None or pa.get("ecorr_toa") is not None


# mutant -> does the case exercise the path it breaks
MUTANTS = {
    "last_bin_dropped": lambda c: c["pa"]["rn_k"] > 0,
    "last_group_unclamped": lambda c: c["pa"]["rn_k"] % 4 != 0,
    "bins_from_12_swapped": lambda c: c["pa"]["rn_k"] > 12,
    "bracket_j_for_j_plus_1": lambda c: c["pa"]["gw_npts"] > 0,
    "ecorr_one_epoch_on": lambda c: c["pa"].get("ecorr_toa") is not None,
    "ecorr_branch_swapped": lambda c: c["pa"].get("ecorr_toa") is not None,
    "ecorr_ep0_off_by_one": lambda c: c["pa"].get("ecorr_toa") is not None and bool(np.any(c["pa"]["tile_epn"] > 0)),
    "wn_z1_z2_swapped": lambda c: c["pa"].get("wn_a") is not None,
    "clamped_lane_written_to_count": lambda c: bool(np.any(c["pa"]["tile_count"] < sc.TILE)),
    "row_R_counter_into_row_R_minus_1": lambda c: c["R"] % 16 != 0 and _draws(c),
    "high_word_of_realisation_dropped": lambda c: c["r0"] + c["R"] - 1 >= 2 ** 32 and _draws(c),
    "stream_psr_of_previous_tile": lambda c: _draws(c) and bool(np.any(c["pa"]["tile_psr"] != np.roll(c["pa"]["tile_psr"], 1))),
}


# rng_fast = 1: a mutant that only replaces a deviate z by another, z', errs by amplitude |z - z'| where the bound is at least
# 2e-5 amplitude - no operand can take the ratio beyond |z - z'| / 2e-5 < 1e6.  There the condition is what that bound leaves:
# |z - z'| > 0.06 = 3 amplitudes (wa, wb, ecorr at one TOA) x 2e-5 x 1e3 at some element - three orders, not six.  Every other
# mutant meets 1e6 in those cases too, at the TOAs the cases leave without noise.
DEVIATE_ONLY = {"ecorr_one_epoch_on", "ecorr_branch_swapped", "ecorr_ep0_off_by_one", "wn_z1_z2_swapped",
                "row_R_counter_into_row_R_minus_1", "high_word_of_realisation_dropped", "stream_psr_of_previous_tile"}
FAST_DEVIATE_FACTOR = 1e3


def test_the_cases_are_the_ones_asked_for():
    ks = {kw.get("K", 60) for _, kw in sc.ALL}
    assert set(sc.KS) <= ks and {r for _, kw in sc.ALL for r in [kw.get("R", 17)]} >= set(sc.RS)
    assert sc.tiles_of(sc.COUNTS)[1].shape[0] == 18 and sum(sc.COUNTS) == 2788
    seen = {m: 0 for m in MUTANTS}
    for _, kw in sc.ALL:
        c = sc.make_case(**kw)
        for m, on in MUTANTS.items():
            seen[m] += bool(on(c))
    assert all(v >= 3 for v in seen.values()), seen


@pytest.mark.parametrize("group,kw", sc.ALL, ids=sc.IDS)
def test_fp64_passes_and_every_mutant_fails(group, kw):
    case = sc.make_case(**kw)
    ref, bound = synth_reference(case["pa"], case["seed"], case["r0"], case["R"], single=case["single"], fast=case["fast"])
    assert ref.shape == bound.shape == (case["R"], case["pa"]["n_toa"])
    in_tile = np.zeros(case["pa"]["n_toa"], dtype=bool)
    for s, c in zip(case["pa"]["tile_start"], case["pa"]["tile_count"]):
        in_tile[s:s + c] = True
    assert np.all(np.isfinite(ref[:, in_tile])) and np.all(np.isnan(ref[:, ~in_tile])) and np.all(np.isnan(bound[:, ~in_tile]))
    honest = excess(evaluate(case), ref, bound)
    print(f"{group} {kw}: fp64 NumPy at {honest:.3f} of the bound")
    assert honest <= 1.0
    for m, on in MUTANTS.items():
        if on(case):
            x = excess(evaluate(case, m), ref, bound)
            assert x >= (FAST_DEVIATE_FACTOR if case["fast"] and m in DEVIATE_ONLY else 1e6), (m, x)
