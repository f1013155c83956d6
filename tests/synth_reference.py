"""Host reference of the fused synthesis pass (pta_engine_synth), evaluated in 80-bit long double from the contract in
include/pta_replicator_amd.h ("fused engine") - test infrastructure, not product code, and not a transcription of any kernel:

    out[r, i] = sum_k Ft[k, i] coef[r, a, k]
              + (G[r, a, j + 1] - G[r, a, j]) w[i] + G[r, a, j]                    j = gw_jlo[i]
              + wa[i] z1 + wb[i] z2           (pair idx_in_psr[i] of stream (WN, a), realisation r0 + r)
              + ecorr[i] z                    (branch e & 1 of pair e >> 1 of stream (ECORR, a), e = epoch_of[i])
              + det[i]

with a = the pulsar of the tile that holds TOA i; a TOA in no tile has no value (NaN).  The deviates are the Philox uniforms of
oracle/philox_ref.py pushed through a long double Box-Muller (box_muller_ld).

A plan is a dict of NumPy arrays named like the members of pta_engine_plan: n_toa, n_psr, tile_psr, tile_start, tile_count,
idx_in_psr, Ft [K, >= n_toa] (the leading dimension is the device's business), rn_coef [R, P, K], gw_G [R, P, npts], gw_jlo, gw_w,
wn_a, wn_b (or wn_c), epoch_of, ecorr_toa, det; a signal whose arrays are None (or missing) is absent.

The bound that comes with the reference is derived, not tuned.  u = 2^-53; every product and sum of an fp64 evaluation rounds once:
  * a K-term dot product, FMA or not, in ANY order of summation:       K u sum_k |Ft coef|                      (Higham, ASNA 3.1)
  * (G1 - G0) w + G0: three roundings of quantities <= |G0| + |G1|:    4 u (|G0| + |G1|)
  * a deviate within 6 ulp <= 12 u |z| of the long double one (the project's own assertion,
    test_device_deviates_within_a_few_ulp_of_an_80_bit_box_muller), its product with the amplitude and the sum of the two
    products:                                                           14 u (|wa z1| + |wb z2| + |ecorr z|)
  * the four sums that join the five terms, and the second-order slack of everything above:   6 u S,   S = sum of |every term|
rng_fast = 1 replaces the deviates' share by 2e-5 (|wa| + |wb| + |ecorr|), the figure test_fast_rng_math_mode asserts against
philox_ref.normal_pairs(fast=True), which is then also where the reference takes its deviates from."""
import numpy as np

from oracle import philox_ref

L = np.longdouble
U = 2.0 ** -53
HAVE_LONG_DOUBLE = np.finfo(L).nmant >= 63


def box_muller_ld(u1, u2):
    """(z0, z1) in long double of the uniforms of philox_ref.uniform_pairs: sqrt(-2 ln u1) (cos, sin)(2 pi u2), the angle reduced
    exactly to the nearest quarter turn as the device does."""
    rad = np.sqrt(L(-2) * np.log(u1.astype(L)))
    q = np.rint(4 * u2); x = (u2.astype(L) - L(0.25) * q.astype(L)) * (L(2) * np.arccos(L(-1)))
    sr, cr = np.sin(x), np.cos(x); k = q.astype(np.int64) & 3
    return rad * np.choose(k, [cr, -sr, -cr, sr]), rad * np.choose(k, [sr, cr, -sr, -cr])


# deviates are a pure function of (seed, realisation, stream, pair): computed once per block of pairs and kept for every case of a
# test session that asks again.  mode: "ld" long double Box-Muller, "f64" philox_ref's libm one, "fast" its fp32 twin of rng_fast = 1
_BLOCK = 256
_cache = {}


def _block(seed, real, stream, b, mode):
    key = (seed, real, stream, b, mode)
    z = _cache.get(key)
    if z is None:
        if mode == "ld":
            z = box_muller_ld(*philox_ref.uniform_pairs(seed, real, stream, _BLOCK, pair0=b * _BLOCK))
        else:
            z = philox_ref.normal_pairs(seed, real, stream, _BLOCK, pair0=b * _BLOCK, fast=mode == "fast")
        _cache[key] = z
    return z


def deviate_pairs(seed, real, stream, pairs, mode="ld"):
    """(z0[n], z1[n]): both branches of the Box-Muller pairs `pairs` (any order, repeats allowed; taken modulo 2^32 like the device's
    counter word) of `stream` for realisation `real` (modulo 2^64)."""
    real = int(real) & 0xFFFFFFFFFFFFFFFF
    pairs = np.asarray(pairs, dtype=np.int64) & 0xFFFFFFFF
    if pairs.size == 0:
        e = np.zeros(0, dtype=L if mode == "ld" else np.float64)
        return e, e
    b = pairs // _BLOCK
    b0 = int(b.min())
    if b0 == int(b.max()):
        z0, z1 = _block(seed, real, stream, b0, mode)
        o = pairs - b0 * _BLOCK
        return z0[o], z1[o]
    z0 = np.empty(pairs.shape, dtype=L if mode == "ld" else np.float64)
    z1 = np.empty_like(z0)
    for bb in np.unique(b):
        m = b == bb
        y0, y1 = _block(seed, real, stream, int(bb), mode)
        o = pairs[m] - int(bb) * _BLOCK
        z0[m], z1[m] = y0[o], y1[o]
    return z0, z1


def wn_pair_and_branch(idx):
    """single-deviate white noise (pta_engine_plan.wn_c): TOA idx takes branch (idx >> 4) & 1 of pair idx & ~16."""
    idx = np.asarray(idx, dtype=np.int64)
    return idx & ~np.int64(16), (idx >> 4) & 1


def synth_reference(plan_arrays, seed, r0, R, single=False, fast=False):
    """(ref, bound), both [R, n_toa]: the long double value of every (realisation, TOA) of the plan and the error an fp64 evaluation
    of it is allowed (module docstring).  NaN where a TOA lies in no tile."""
    pa = plan_arrays
    n = int(pa["n_toa"])
    mode = "fast" if fast else "ld"
    ref = np.full((R, n), np.nan, dtype=L)
    bound = np.full((R, n), np.nan, dtype=L)
    Ft, coef, G = pa.get("Ft"), pa.get("rn_coef"), pa.get("gw_G")
    wa, wb, wc = pa.get("wn_a"), pa.get("wn_b"), pa.get("wn_c")
    ecv, det = pa.get("ecorr_toa"), pa.get("det")
    assert (wc is not None) == bool(single) and not (single and wa is not None)
    for a, s, c in zip(pa["tile_psr"], pa["tile_start"], pa["tile_count"]):
        a, sl = int(a), slice(int(s), int(s) + int(c))
        val = np.zeros((R, int(c)), dtype=L)      # the value
        S = np.zeros_like(val)                    # sum of |every term|
        E = np.zeros_like(val)                    # the terms' own shares of the bound, in units of u
        Z = np.zeros_like(val)                    # rng_fast: sum of the amplitudes a deviate multiplies
        if Ft is not None and coef is not None:
            K = coef.shape[2]
            F, cf = Ft[:K, sl].astype(L), coef[:R, a, :].astype(L)
            mag = np.abs(cf) @ np.abs(F)
            val += cf @ F
            S += mag
            E += K * mag
        if G is not None:
            j, w = pa["gw_jlo"][sl].astype(np.int64), pa["gw_w"][sl].astype(L)
            g0, g1 = G[:R, a, :][:, j].astype(L), G[:R, a, :][:, j + 1].astype(L)
            val += (g1 - g0) * w + g0
            S += np.abs(g1 - g0) * np.abs(w) + np.abs(g0)
            E += 4 * (np.abs(g0) + np.abs(g1))
        for r in range(R):
            dev = np.zeros(int(c), dtype=L)       # sum of |amplitude x deviate|
            if wa is not None or wc is not None:
                strm = philox_ref.stream_id(philox_ref.STREAM_WN, a)
                idx = pa["idx_in_psr"][sl]
                if single:
                    pair, br = wn_pair_and_branch(idx)
                    z0, z1 = deviate_pairs(seed, r0 + r, strm, pair, mode)
                    t1, t2 = wc[sl].astype(L) * np.where(br == 1, z1, z0), L(0)
                    Z[r] += np.abs(wc[sl])
                else:
                    z1, z2 = deviate_pairs(seed, r0 + r, strm, idx, mode)
                    t1, t2 = wa[sl].astype(L) * z1, wb[sl].astype(L) * z2
                    Z[r] += np.abs(wa[sl]) + np.abs(wb[sl])
                val[r] += t1 + t2
                dev += np.abs(t1) + np.abs(t2)
            if ecv is not None:
                e = pa["epoch_of"][sl].astype(np.int64)
                z0, z1 = deviate_pairs(seed, r0 + r, philox_ref.stream_id(philox_ref.STREAM_ECORR, a), e >> 1, mode)
                t = ecv[sl].astype(L) * np.where((e & 1) == 1, z1, z0)
                val[r] += t
                dev += np.abs(t)
                Z[r] += np.abs(ecv[sl])
            S[r] += dev
            if not fast:
                E[r] += 14 * dev
        if det is not None:
            val += det[sl].astype(L)
            S += np.abs(det[sl].astype(L))
        ref[:, sl] = val
        bound[:, sl] = L(U) * (E + 6 * S) + (L(2e-5) * Z if fast else 0)
    return ref, bound.astype(np.float64)
