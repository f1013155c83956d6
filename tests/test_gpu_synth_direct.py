"""pta_engine_synth called directly, on plans this test builds by hand (tests/synth_cases.py), against the long double host reference
of the header's contract (tests/synth_reference.py): every variant that has a kernel (0, 1, 2, 6 and the hooks 16, 32, 48, 64) within
the derived fp64 bound at every element, everything outside the view and every TOA in no tile untouched.  The absolute anchor of the
edge shapes - the bit-identity tests (test_gpu_synth_copies / _wide / _lean) compare the kernel's copies with one another.

  B.1  tiles ending one short of, at and one past every wave and pair boundary, full tiles followed by a short one; K over every residue
       of the group of four bins and of the rotation's trip of twelve; R in (1, 15, 16, 17, 33); realisation counters below, across and
       beyond 2^32; every signal absent on its own, ECORR only, red noise only; sub-plans of 1, 7, 9 tiles out of pulsar order
  B.2  ECORR epochs straddling tiles with an odd / even first epoch, exactly PTA_ENGINE_EPMAX pairs, one more (per-TOA path, a third of
       the amplitudes zero), shuffled inside a tile
  B.3  GWB grids of 2, 3, 601 samples with brackets 0 and npts - 2 and weights exactly 0 and 1; single-deviate white noise; arbitrary
       pair indices; rng_fast = 1 against its own bound
  B.4  the host guard of the 32-bit lane offsets: K = 2, 4 at the largest ldf it accepts (lane offsets beyond 2^31; K = 2 also the
       tail loop's modular step back) and the smallest it rejects (index products), in one 4.3 GB buffer of which only the used columns
       are written
  B.5  pta_engine_rn_coef: amp z against the long double deviates, 14 u |amp z|

Worst |got - ref| / bound measured on the MI355X over every case and variant of a group (1 = at the bound; the tests print it per
case, `pytest -s`):
  B.1  K list 0.256   (R, seed, r0) lists 0.085   plans and sub-plans 0.308
  B.2  0.230          B.3  0.183 (rng_fast = 1: 0.06 of its own bound)
  B.4  0.163          B.5  0.307
The same figure for an fp64 NumPy evaluation with libm deviates (tests/test_synth_reference_host.py) is 0.03 to 0.26 over the cases:
the bound has a factor of three or more in hand, as a worst-case bound over up to 62 roundings should, and a wrong O(1) term would
miss it by thirteen orders."""
import ctypes

import numpy as np
import pytest

import synth_cases as sc
from oracle import philox_ref
from synth_reference import HAVE_LONG_DOUBLE, L, U, deviate_pairs, synth_reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")]

VARIANTS = (0, 1, 2, 6, 16, 32, 48, 64)
PAD_LEFT, PAD_COLS = 3, 6


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert (_lib.ENGINE_TILE, _lib.ENGINE_EPMAX) == (sc.TILE, sc.EPMAX)
    return dict(torch=torch, lib=_lib, dv=dv)


def device_plan(gpu, pa, R, fast=False, Ft_dev=None, ldf=None):
    """(_lib.EnginePlan, the tensors it points at) for a plan of NumPy arrays.  The design matrix gets ldf = n_toa + 3 with NaN in the
    three columns no TOA owns, unless the caller brings its own device buffer and leading dimension (B.4)."""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    n = pa["n_toa"]
    hold = {}

    def put(key, make):
        x = pa.get(key)
        if x is None:
            return None
        hold[key] = make(x)
        return hold[key].data_ptr()
    pl = lib.EnginePlan()
    pl.n_toa, pl.n_psr, pl.rn_k, pl.gw_npts, pl.tnequad, pl.n_tiles = n, pa["n_psr"], pa["rn_k"], pa["gw_npts"], 0, len(pa["tile_psr"])
    for k in ("tile_psr", "tile_start", "tile_count", "tile_ep0", "tile_epn", "idx_in_psr", "gw_jlo", "epoch_of"):
        setattr(pl, k, put(k, dv.i32))
    for k in ("gw_G", "gw_w", "wn_a", "wn_b", "wn_c", "ecorr_toa", "det"):
        setattr(pl, k, put(k, dv.f64))
    pl.Ft, pl.ldf, pl.rn_coef = None, 0, None
    if pa["rn_k"]:
        assert pa["rn_coef"].shape == (R, pa["n_psr"], pa["rn_k"])
        pl.rn_coef = put("rn_coef", dv.f64)
        if Ft_dev is None:
            ldf = n + 3
            F = np.full((pa["rn_k"], ldf), np.nan)
            F[:, :n] = pa["Ft"]
            hold["Ft"] = dv.f64(F)
            pl.Ft = hold["Ft"].data_ptr()
        else:
            assert Ft_dev.numel() >= (pa["rn_k"] - 1) * ldf + n and ldf >= n
            torch.as_strided(Ft_dev, (pa["rn_k"], n), (ldf, 1)).copy_(dv.f64(pa["Ft"]))
            pl.Ft = Ft_dev.data_ptr()
        pl.ldf = ldf
    pl.rng_fast = 1 if fast else 0
    return pl, hold


def run_variant(gpu, pl, variant, seed, r0, R, n):
    """one launch into the view [R, n] at column 3 of a NaN-filled [R + 1, n + 6] buffer: rows 8-byte, never 16-byte aligned throughout"""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    big = dv.empty((R + 1, n + PAD_COLS))
    big.fill_(float("nan"))
    view = big[:R, PAD_LEFT:PAD_LEFT + n]
    assert view.stride(0) == n + PAD_COLS and view.data_ptr() % 16 == 8
    pl.synth_variant = variant
    lib.call("pta_engine_synth", ctypes.byref(pl), seed, r0, R, ctypes.c_void_p(view.data_ptr()), n + PAD_COLS, dv.stream_ptr())
    torch.cuda.synchronize()
    return big.cpu().numpy()


def worst_ratio(big, ref, bound, what):
    """asserts the contract of one launch and returns max |got - ref| / bound"""
    R, n = ref.shape
    view = big[:R, PAD_LEFT:PAD_LEFT + n]
    outside = big.copy()
    outside[:R, PAD_LEFT:PAD_LEFT + n] = np.nan
    hole = np.isnan(ref)
    assert np.all(np.isnan(outside)), (what, "written outside the view")
    assert np.all(np.isnan(view[hole])), (what, "a TOA in no tile was written")
    assert np.all(np.isfinite(view[~hole])), (what, "not finite")
    err = np.abs(view.astype(L) - ref).astype(np.float64)[~hole]
    b = bound[~hole]
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    assert np.all(err <= b), (what, worst, int(np.argmax(ratio)))
    return worst


def check_case(gpu, case, group, variants=VARIANTS, Ft_dev=None, ldf=None):
    pa, seed, r0, R = case["pa"], case["seed"], case["r0"], case["R"]
    ref, bound = synth_reference(pa, seed, r0, R, single=case["single"], fast=case["fast"])
    pl, hold = device_plan(gpu, pa, R, fast=case["fast"], Ft_dev=Ft_dev, ldf=ldf)
    worst = 0.0
    for v in variants:
        if v == 6 and case["single"]:     # the single-deviate white noise exists in the MFMA kernel only: refused, not replaced
            pl.synth_variant = 6
            with pytest.raises(gpu["lib"].PtaError):
                run_variant(gpu, pl, 6, seed, r0, R, pa["n_toa"])
            continue
        worst = max(worst, worst_ratio(run_variant(gpu, pl, v, seed, r0, R, pa["n_toa"]), ref, bound, (group, v)))
    print(f"SYNTH_DIRECT {group} worst |got - ref| / bound = {worst:.4f}")
    del hold
    return worst


@pytest.mark.parametrize("group,kw", sc.ALL, ids=sc.IDS)
def test_every_variant_within_the_bound(gpu, group, kw):
    check_case(gpu, sc.make_case(**kw), group)


# ---------------------------------------------------------------- B.4 ----------------
def guard_ldf_max(K, R, P):
    """the largest ldf for which pta_engine_synth still takes the 32-bit lane offsets (its expression: ldf < 2^28 and
    (K ldf + PTA_ENGINE_TILE) 8 + 24 < 2^32 and R P K 8 < 2^32)"""
    assert R * P * K * 8 < 2 ** 32
    ldf = min(2 ** 28 - 1, ((2 ** 32 - 24 - 1) // 8 - sc.TILE) // K)
    assert (K * ldf + sc.TILE) * 8 + 24 < 2 ** 32 <= (K * (ldf + 1) + sc.TILE) * 8 + 24 or ldf == 2 ** 28 - 1
    return ldf


@pytest.fixture(scope="module")
def four_gigabytes(gpu):
    torch = gpu["torch"]
    numel = max(K * (guard_ldf_max(K, 17, 1) + 1) for K in (2, 4))
    assert 4.29e9 < numel * 8 < 4.3e9
    buf = torch.empty((numel,), dtype=torch.float64, device="cuda")    # uninitialised: only the used columns are written
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("rejected", [0, 1], ids=["largest_accepted", "smallest_rejected"])
def test_lane_offset_guard(gpu, four_gigabytes, K, rejected):
    """one pulsar of 257 TOAs (a full tile: the 16-byte loads, and a tile of one clamped lane), R = 17; every address lies inside
    the buffer: (K - 1) ldf + 257 <= K (ldf_max + 1) doubles"""
    case = sc.make_case(K=K, R=17, counts=(257,), seed=sc.SEEDS[1][0], r0=sc.SEEDS[1][1])
    ldf = guard_ldf_max(K, 17, 1) + rejected
    # (the byte offset of the tile's last TOA in the last bin is beyond 2^31)
    assert ((K - 1) * ldf + 255) * 8 > 2 ** 31 and (K - 1) * ldf + 257 <= four_gigabytes.numel()
    check_case(gpu, case, "B4_guard", Ft_dev=four_gigabytes, ldf=ldf)


# ---------------------------------------------------------------- B.5 ----------------
@pytest.mark.parametrize("R,P,K", [(1, 1, 2), (17, 5, 58), (33, 3, 60)])
def test_rn_coef_direct(gpu, R, P, K):
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    seed, r0 = 0x9E3779B97F4A7C15, 2 ** 32 - 3
    rng = np.random.default_rng([R, P, K])
    amp = rng.standard_normal((P, K))
    amp[rng.random((P, K)) < 0.05] = 0.0
    d_amp, d_coef = dv.f64(amp), dv.empty((R, P, K))
    d_coef.fill_(float("nan"))
    lib.call("pta_engine_rn_coef", seed, r0, R, P, K, dv.ptr(d_amp), dv.ptr(d_coef), 0, dv.stream_ptr())
    torch.cuda.synchronize()
    got = d_coef.cpu().numpy()
    ref = np.empty((R, P, K), dtype=L)
    for r in range(R):
        for a in range(P):
            z0, z1 = deviate_pairs(seed, r0 + r, philox_ref.stream_id(philox_ref.STREAM_RN, a), np.arange(K // 2))
            ref[r, a, 0::2], ref[r, a, 1::2] = amp[a, 0::2] * z0, amp[a, 1::2] * z1
    err = np.abs(got.astype(L) - ref).astype(np.float64)
    bound = (14 * U * np.abs(ref)).astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"SYNTH_DIRECT B5_rn_coef worst |got - ref| / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.4f}")


def test_rn_coef_refuses_odd_K(gpu):
    dv, lib = gpu["dv"], gpu["lib"]
    d_amp, d_coef = dv.zeros((2, 3)), dv.zeros((2, 2, 3))
    with pytest.raises(lib.PtaError):
        lib.call("pta_engine_rn_coef", 1, 0, 2, 2, 3, dv.ptr(d_amp), dv.ptr(d_coef), 0, dv.stream_ptr())
