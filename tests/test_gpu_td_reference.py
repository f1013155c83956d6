"""The dense TD path on the GPU - assembly, every factorisation entry point and schedule the engine can select, the draw - held to
the long double residuals and derived bounds of tests/td_reference.py on the hand-built inputs of tests/td_cases.py (run with
-m gpu on an MI355X).  No factor is compared with another factor here: a case passes when info == 0, the lower triangle is finite,
the componentwise residual |A - L L^T| stays inside the bound of the schedule's class ((s): conventional; (w): product with the
inverse of the diagonal blocks) and a second run returns the same bits.  On failure the worst fraction of the bound is reported.

A residual costs seconds of long double arithmetic at the larger orders; it depends on (A, L) alone, so it is computed once per
distinct factor: batches of 1, 3 and 5 share their leading matrices, and schedules that only reorder launches return the same bits.
MEASURED (printed with -s) collects the worst fraction per entry point and family; DESIGN.md 4.2.1 quotes it."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import td_cases as tc
import td_reference as tr
from oracle import philox_ref
from td_reference import HAVE_LONG_DOUBLE, LD, U

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")]

ORDER = ("Q", "Lo", "W")        # matrix b of a batch: family ORDER[b % 3], seed b // 3
MEASURED = {}
_judged = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(torch=torch, lib=_lib, dv=dv, s=dv.stream_ptr())


@functools.lru_cache(maxsize=None)
def _matrix(fam, n, seed):
    return tc.family(fam, n, seed)["A"]


def _batch(n, B, fams=ORDER):
    return [(fams[b % len(fams)], _matrix(fams[b % len(fams)], n, b // len(fams))) for b in range(B)]


def _judge(entry, fam, A, L, cls, panels=None, extra=None):
    """fraction of its bound the factor L of A fills (cached per distinct (A, L)); records the worst per (entry point, family)"""
    key = (hashlib.sha1(np.ascontiguousarray(A).tobytes()).hexdigest(), hashlib.sha1(np.ascontiguousarray(L).tobytes()).hexdigest(), cls,
           tuple(panels) if panels else None)
    if key not in _judged:
        D, S = tr.cholesky_residual(A, L)
        b = tr.bound_s(S) if cls is None else tr.bound_w(L, S, cls, panels)
        if extra is not None:
            b = b + extra
        _judged[key] = (tr.rho_c(D, b) * U, tr.rho_n(D, A))
    fill, rn = _judged[key]
    m = MEASURED.setdefault((entry, fam), [0.0, 0.0])
    m[0], m[1] = max(m[0], fill), max(m[1], rn)
    print(f"{entry} {fam} n={A.shape[0]}: fraction of the bound {fill:.4f}, rho_n {rn:.1f}")
    return fill


def _check(entry, mats, Ls, info, cls, panels_of, extra=None):
    assert not np.any(info), info
    for b, ((fam, A), L) in enumerate(zip(mats, Ls)):
        assert np.all(np.isfinite(L)), (entry, b, fam)
        fill = _judge(entry, fam, A, L, cls, panels_of(A.shape[0]) if panels_of else None, None if extra is None else extra[b])
        assert fill <= 1.0, f"{entry}: matrix {b} ({fam}, n = {A.shape[0]}) fills {fill:.3f} of its bound"


def _uniform(gpu, mats, fl, workspace=True):
    """pta_potrf_batched_ws (or _ex) on a uniform batch: leading-dimension and stride slack, NaN above the diagonals, NaN workspace;
    two runs, bit-identical; returns the lower factors and info"""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    B, n = len(mats), mats[0][1].shape[0]
    ld = n + (n & 1) + 2
    buf = np.full((B, n + 1, ld), np.nan)
    for b, (_, A) in enumerate(mats):
        buf[b, :n, :n] = np.tril(A) + np.triu(np.full((n, n), np.nan), 1)
    outs = []
    for rep in range(2):
        Ad = dv.f64(buf)
        info = dv.zeros((B,), dtype=torch.int32)
        if workspace:
            need = int(lib.lib.pta_potrf_workspace_doubles(n, B, fl))
            assert need > 0
            work = dv.empty((need,))
            work.fill_(float("nan"))
            lib.call("pta_potrf_batched_ws", dv.ptr(Ad), n, ld, (n + 1) * ld, B, dv.ptr(info), fl, dv.ptr(work), need, gpu["s"])
        else:
            lib.call("pta_potrf_batched_ex", dv.ptr(Ad), n, ld, (n + 1) * ld, B, dv.ptr(info), fl, gpu["s"])
        outs.append((np.tril(Ad.cpu().numpy()[:, :n, :n]), info.cpu().numpy()))
    assert np.array_equal(outs[0][1], outs[1][1])
    if not outs[0][1].any():
        assert np.array_equal(outs[0][0], outs[1][0]), "second run differs"
    return list(outs[0][0]), outs[0][1]


def _ragged(gpu, mats, fl):
    """pta_potrf_ragged: slack in every other leading dimension and between matrices, NaN above the diagonals, NaN workspace; two runs"""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    B = len(mats)
    n = np.array([A.shape[0] for _, A in mats], dtype=np.int32)
    ld = ((n.astype(np.int64) + 15) // 16 * 16 + 16 * (np.arange(B) % 2)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n.astype(np.int64) * ld + 32)])[:-1].astype(np.int64)
    buf = np.full(int(off[-1] + n[-1] * ld[-1] + 32), np.nan)
    for b, (_, A) in enumerate(mats):
        v = buf[off[b]:off[b] + n[b] * ld[b]].reshape(n[b], ld[b])
        v[:, :n[b]] = np.tril(A) + np.triu(np.full(A.shape, np.nan), 1)
    plan = np.zeros(int(lib.lib.pta_potrf_ragged_plan_words(B)), dtype=np.int64)
    need = ctypes.c_int64(0)
    lib.call("pta_potrf_ragged_plan", dv.hptr(n), dv.hptr(off), dv.hptr(ld), B, fl, dv.hptr(plan), ctypes.byref(need))
    plan_d = dv.i64(plan)
    outs = []
    for rep in range(2):
        Ad = dv.f64(buf)
        work = dv.empty((max(need.value, 1),))
        work.fill_(float("nan"))
        info = dv.zeros((B,), dtype=torch.int32)
        lib.call("pta_potrf_ragged", dv.ptr(Ad), dv.hptr(plan), dv.ptr(plan_d), dv.ptr(info), dv.ptr(work), need.value, gpu["s"])
        out = Ad.cpu().numpy()
        outs.append(([np.tril(out[off[b]:off[b] + n[b] * ld[b]].reshape(n[b], ld[b])[:, :n[b]]) for b in range(B)], info.cpu().numpy()))
    assert np.array_equal(outs[0][1], outs[1][1])
    if not outs[0][1].any():
        for x, y in zip(outs[0][0], outs[1][0]):
            assert np.array_equal(x, y), "second run differs"
    return outs[0]


@pytest.mark.parametrize("B", tc.WS_BATCHES)
@pytest.mark.parametrize("sched", tc.WS_SCHEDULES)
@pytest.mark.parametrize("n", tc.WS_ORDERS)
def test_workspace_scheme_256_column_panels(gpu, n, sched, B):
    """pta_potrf_batched_ws, PTA_POTRF_NB(1): every schedule the engine can select on Q, Lo and W, inside bound (w) with 128-column groups"""
    lib = gpu["lib"]
    mats = _batch(n, B)
    Ls, info = _uniform(gpu, mats, tc.flag_bits(lib, sched) | lib.POTRF_NB(1))
    _check("ws", mats, Ls, info, 128, lambda m: tr.panels_uniform(m, 256))


@pytest.mark.parametrize("sched", ["LEFT", "0"])
def test_workspace_scheme_default_chains(gpu, sched):
    """eight matrices and no PTA_POTRF_CHAINS: the default is two chains from B = 8 on and one below (pta_potrf_impl), which the other
    batches (1, 3, 5) and the explicit CHAINS schedules never take.  Inside bound (w), and bit for bit what one chain returns: the
    chains only divide the matrices among streams."""
    lib = gpu["lib"]
    mats = _batch(258, 8)
    fl = tc.flag_bits(lib, sched) | lib.POTRF_NB(1)
    Ls, info = _uniform(gpu, mats, fl)
    _check("ws", mats, Ls, info, 128, lambda m: tr.panels_uniform(m, 256))
    L1, info1 = _uniform(gpu, mats, fl | lib.POTRF_CHAINS(1))
    assert not info1.any() and all(np.array_equal(x, y) for x, y in zip(Ls, L1))


@pytest.mark.parametrize("n,sched", tc.WIDE_CASES)
def test_workspace_scheme_default_panels(gpu, n, sched):
    """the default 1024-column panels just above one panel: a first panel of 1026 columns and of 1034 + 256; one matrix per case"""
    mats = _batch(n, 1, fams=("Lo",) if n == 1026 else ("Q",))
    Ls, info = _uniform(gpu, mats, tc.flag_bits(gpu["lib"], sched))
    _check("ws1024", mats, Ls, info, 128, lambda m: tr.panels_uniform(m, 1024))


@pytest.mark.parametrize("flags", tc.EX_FLAGS)
@pytest.mark.parametrize("n", tc.EX_ORDERS)
def test_potrf_batched_ex_without_workspace(gpu, n, flags):
    """pta_potrf_batched_ex: the 64-column product solves inside bound (w), substitution and the VALU cross-check inside bound (s) -
    these two also on X, cond 1e12"""
    conventional = flags in ("SUBSTITUTION", "VALU")
    mats = _batch(n, 4 if conventional else 3, fams=ORDER + ("X",) if conventional else ORDER)
    Ls, info = _uniform(gpu, mats, tc.flag_bits(gpu["lib"], flags), workspace=False)
    _check("ex " + flags, mats, Ls, info, None if conventional else 64, None)


@pytest.mark.parametrize("flags", tc.RAGGED_FLAGS)
@pytest.mark.parametrize("orders", tc.RAGGED_ORDERS)
def test_potrf_ragged(gpu, orders, flags):
    """pta_potrf_ragged, 256-column panels, families mixed within the batch: entries at block boundaries, inside blocks, orders below
    one block"""
    lib = gpu["lib"]
    mats = [(ORDER[b % 3], _matrix(ORDER[b % 3], n, 0)) for b, n in enumerate(orders)]
    Ls, info = _ragged(gpu, mats, tc.flag_bits(lib, flags) | lib.POTRF_NB(1))
    _check("ragged", mats, Ls, info, 128, lambda m: tr.panels_ragged(m, 256))


@pytest.mark.parametrize("P", tc.ORF_ORDERS)
def test_orf_factor_per_realisation(gpu, P):
    """pta_gwb_orf_factor (conventional: bound (s)) on all four families: one basis matrix and clm = a power of two per realisation,
    so that 2 clm basis is exact and realisation r factors 2 clm_r A; five realisations (four per workgroup and one)"""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    clm = np.array([0.5, 1.0, 0.25, 0.5, 2.0])
    for fam in tc.FAMILIES:
        A = _matrix(fam, P, 0)
        A = np.tril(A) + np.tril(A, -1).T
        dA, dc = dv.f64(A), dv.f64(clm)
        outs = []
        for rep in range(2):
            M = dv.f64(np.full((len(clm), P, P), np.nan))
            info = dv.zeros((len(clm),), dtype=torch.int32)
            lib.call("pta_gwb_orf_factor", dv.ptr(dA), 1, P, dv.ptr(dc), 1, len(clm), dv.ptr(M), dv.ptr(info), gpu["s"])
            outs.append((M.cpu().numpy(), info.cpu().numpy()))
        assert np.array_equal(outs[0][0], outs[1][0]), "second run differs"
        assert np.all(np.triu(outs[0][0], 1) == 0)
        _check("orf_factor", [(fam, 2 * c * A) for c in clm], list(outs[0][0]), outs[0][1], None, None)


# ---- fused assembly + factorisation ----
@functools.lru_cache(maxsize=None)
def _fused_inputs(n, kf, ecorr):
    """two pulsars (Q- and Lo-like amplitudes), 64 design columns of which kf are used, TOAs shuffled; the long double covariances"""
    ds, refs = [], []
    for b, fam in enumerate(("Q", "Lo")):
        d = tc.td_inputs(n, 40 + b, **{**tc._TD[fam], "ecorr": 1e-7 if ecorr else None}, ncomp=32, shuffle=True)
        d["Ft"], d["phi"] = d["Ft"][:kf], d["phi"][:kf]
        ds.append(d)
        refs.append(tr.cov_reference(d["Ft"] if kf else None, d["phi"], d["sigma2"], d["epoch_of"], d["ecorr2"]))
    return ds, refs


def _fused(gpu, ds, n, kf, fl):
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    B = len(ds)
    Fr = np.zeros((B * n, 64))
    Gr = np.zeros((B * n, 64))
    for b, d in enumerate(ds):
        Fr[b * n:(b + 1) * n, :kf] = d["Ft"].T
        Gr[b * n:(b + 1) * n, :kf] = -(d["phi"][None, :] * d["Ft"].T)
    sig = np.concatenate([d["sigma2"] for d in ds])
    ec = ds[0]["epoch_of"] is not None
    dF, dG, dS = dv.f64(Fr), dv.f64(Gr), dv.f64(sig)
    dE = dv.i32(np.concatenate([d["epoch_of"] for d in ds])) if ec else None
    dC = dv.f64(np.concatenate([d["ecorr2"] for d in ds])) if ec else None
    ld = n + 2
    need = int(lib.lib.pta_potrf_workspace_doubles(n, B, fl))
    assert need > 0
    outs = []
    for rep in range(2):
        Ad = dv.f64(np.full((B, n + 1, ld), np.nan))
        work = dv.empty((need,))
        work.fill_(float("nan"))
        info = dv.zeros((B,), dtype=torch.int32)
        lib.call("pta_td_assemble_potrf", dv.ptr(dF), dv.ptr(dG), kf, dv.ptr(dS), dv.ptr(dE) if ec else None, dv.ptr(dC) if ec else None,
                 dv.ptr(Ad), n, ld, (n + 1) * ld, B, dv.ptr(info), fl, dv.ptr(work), need, gpu["s"])
        outs.append((np.tril(Ad.cpu().numpy()[:, :n, :n]), info.cpu().numpy()))
    assert np.array_equal(outs[0][1], outs[1][1])
    if not outs[0][1].any():
        assert np.array_equal(outs[0][0], outs[1][0]), "second run differs"
    return list(outs[0][0]), outs[0][1]


@pytest.mark.parametrize("ecorr", [False, True])
@pytest.mark.parametrize("kf", tc.FUSED_KF)
@pytest.mark.parametrize("n", tc.FUSED_ORDERS)
def test_fused_assembly_factorisation(gpu, n, kf, ecorr):
    """pta_td_assemble_potrf: A is the LONG DOUBLE covariance of the operands; the bound is the factor's plus the assembly's"""
    lib = gpu["lib"]
    ds, refs = _fused_inputs(n, kf, ecorr)
    Ls, info = _fused(gpu, ds, n, kf, lib.POTRF_LEFT | lib.POTRF_NB(1))
    mats = [(fam, C) for fam, (C, _) in zip(("Q", "Lo"), refs)]
    _check("fused", mats, Ls, info, 128, lambda m: tr.panels_uniform(m, 256), extra=[tr.cov_bound(mag, kf) for _, mag in refs])


# ---- info ----
@functools.lru_cache(maxsize=None)
def _indefinite(p):
    """Lo at n = 520 with its diagonal entry p lowered by twice pivot p: the pivots before p are untouched, pivot p becomes its own
    negative - far outside rounding (the pivots are >= sigma^2 = 9e-16, their rounding errors below 1e-22)"""
    A = _matrix("Lo", 520, 0).copy()
    L = tc.chol_unblocked(A)
    A[p, p] -= 2 * L[p, p] ** 2
    return A, 2 * L[p, p] ** 2


@pytest.mark.parametrize("p", [5, 136, 400])     # in the narrow first block (8 columns), first column of a 128-column block, last panel
@pytest.mark.parametrize("path", ["uniform", "ragged", "fused"])
def test_info_names_the_first_bad_pivot(gpu, path, p):
    lib = gpu["lib"]
    good, good2 = ("Q", _matrix("Q", 520, 0)), ("W", _matrix("W", 520, 0))
    if path == "uniform":
        _, info = _uniform(gpu, [good, ("Lo", _indefinite(p)[0]), good2], lib.POTRF_LEFT | lib.POTRF_NB(1))
        assert list(info) == [0, p + 1, 0]
    elif path == "ragged":
        _, info = _ragged(gpu, [good, ("Q", _matrix("Q", 258, 0)), ("Lo", _indefinite(p)[0]), good2], lib.POTRF_NB(1))
        assert list(info) == [0, 0, p + 1, 0]
    else:
        ds, _ = _fused_inputs(520, 60, False)
        A = tc.cov_fp64(ds[1])
        bad = dict(ds[1])
        bad["sigma2"] = ds[1]["sigma2"].copy()
        bad["sigma2"][p] -= 2 * tc.chol_unblocked(A)[p, p] ** 2
        _, info = _fused(gpu, [ds[0], bad], 520, 60, lib.POTRF_LEFT | lib.POTRF_NB(1))
        assert list(info) == [0, p + 1]


# ---- assembly ----
@functools.lru_cache(maxsize=None)
def _assembly_inputs(K):
    """five blocks of unsorted TOAs, phi over twelve decades, epoch numbers that repeat from block to block; long double references"""
    blocks = []
    for b, n in enumerate(tc.ASM_ORDERS):
        d = tc.td_inputs(n, 60 + b, log10_A=-13.0, sigma=1e-7, ecorr=1e-7, ncomp=32, shuffle=True)
        d["Ft"] = d["Ft"][:K]
        d["phi"] = 1e-10 * 10.0 ** (-12.0 * np.arange(K) / max(K - 1, 1))
        d["ref"] = tr.cov_reference(d["Ft"], d["phi"], d["sigma2"], d["epoch_of"], d["ecorr2"])
        blocks.append(d)
    return blocks


@pytest.mark.parametrize("kernel", ["tile", "walk", "walk_first"])
@pytest.mark.parametrize("K", tc.ASM_K)
def test_covariance_assembly(gpu, K, kernel):
    """pta_td_cov_assemble_all and pta_td_cov_assemble_walk (epoch_first NULL and given) against the long double covariance"""
    dv, lib = gpu["dv"], gpu["lib"]
    blocks = _assembly_inputs(K)
    ns = np.array(tc.ASM_ORDERS, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    N, P = int(off[-1]), len(ns)
    lds = ((ns + 15) // 16 * 16).astype(np.int32)
    pos = np.concatenate([[0], np.cumsum(ns.astype(np.int64) * lds + 16)]).astype(np.int64)
    Ft = np.concatenate([d["Ft"] for d in blocks], axis=1)
    efirst = np.empty(N, dtype=np.int32)
    for b, d in enumerate(blocks):
        ep = d["epoch_of"].astype(np.int64)
        first = np.full(int(ep.max()) + 1, len(ep), dtype=np.int64)
        np.minimum.at(first, ep, np.arange(len(ep)))
        efirst[off[b]:off[b + 1]] = first[ep]
    dev = dict(Ft=dv.f64(Ft), phi=dv.f64(np.stack([d["phi"] for d in blocks])), s2=dv.f64(np.concatenate([d["sigma2"] for d in blocks])),
               ep=dv.i32(np.concatenate([d["epoch_of"] for d in blocks])), ec=dv.f64(np.concatenate([d["ecorr2"] for d in blocks])),
               pos=dv.i64(pos[:-1]), ld=dv.i32(lds), n=dv.i32(ns), off=dv.i32(off[:-1]), ef=dv.i32(efirst))
    outs = []
    for rep in range(2):
        C = dv.f64(np.full(int(pos[-1]), np.nan))
        common = (dv.ptr(dev["Ft"]), N, K, dv.ptr(dev["phi"]), dv.ptr(dev["s2"]), dv.ptr(dev["ep"]), dv.ptr(dev["ec"]), dv.ptr(C), dv.ptr(dev["pos"]),
                  dv.ptr(dev["ld"]), dv.ptr(dev["n"]), dv.ptr(dev["off"]), P)
        if kernel == "tile":
            lib.call("pta_td_cov_assemble_all", *common, int(ns.max()), gpu["s"])
        else:
            item0 = np.zeros(P + 1, dtype=np.int32)
            total = int(lib.lib.pta_td_cov_walk_items(dv.hptr(ns), P, K, 0, dv.hptr(item0)))
            assert total > 0
            d_item0 = dv.i32(item0)
            lib.call("pta_td_cov_assemble_walk", *common, dv.ptr(d_item0), total, dv.ptr(dev["ef"]) if kernel == "walk_first" else None, 0, gpu["s"])
        outs.append(C.cpu().numpy())
    assert np.array_equal(outs[0], outs[1], equal_nan=True), "second run differs"
    for b, d in enumerate(blocks):
        n = int(ns[b])
        got = outs[0][pos[b]:pos[b] + n * lds[b]].reshape(n, lds[b])[:, :n]
        lo = np.tril_indices(n)
        assert np.all(np.isfinite(got[lo])), (b, n)
        ref, mag = d["ref"]
        fill = tr.rho_c(np.abs(np.tril(np.where(np.isfinite(got), got, 0.0)).astype(LD) - ref), tr.cov_bound(mag, K)) * U
        m = MEASURED.setdefault(("assembly " + kernel, "K"), [0.0, 0.0])
        m[0] = max(m[0], fill)
        print(f"assembly {kernel} K={K} n={n}: fraction of the bound {fill:.4f}")
        assert fill <= 1.0, f"assembly {kernel}: block {b} (n = {n}, K = {K}) fills {fill:.3f} of its bound"


# ---- draw ----
SEED, R0 = 99, 1234567890123


@functools.lru_cache(maxsize=None)
def _draw_factors():
    return [tc.chol_unblocked(_matrix(("Q", "Lo")[b % 2], n, 0)) for b, n in enumerate(tc.DRAW_ORDERS)]


@functools.lru_cache(maxsize=None)
def _drawn(kind, b, m, n):
    return tr.drawn_z(SEED, R0 + m, philox_ref.stream_id(kind, b), n)


def _plan(gpu, Ls, rows_per_real, kind, keep, partial_last):
    """pta_td_plan over host factors (NaN above the diagonals, slack in every other leading dimension)"""
    lib, dv = gpu["lib"], gpu["dv"]
    from pta_replicator_amd.engine_td import _strips
    ns = [L.shape[0] for L in Ls]
    lds = [(n + 1) // 2 * 2 + (2 if b % 2 else 0) for b, n in enumerate(ns)]
    pos = np.concatenate([[0], np.cumsum([n * l for n, l in zip(ns, lds)])]).astype(np.int64)
    buf = np.full(int(pos[-1]), np.nan)
    for b, L in enumerate(Ls):
        v = buf[pos[b]:pos[b] + ns[b] * lds[b]].reshape(ns[b], lds[b])
        il = np.tril_indices(ns[b])
        v[il] = L[il]
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    blk, n0, rows = _strips(ns)
    if partial_last:   # strips at multiples of PTA_TD_STRIP, item_rows = NULL: the partial strip is the last one
        items = sorted([(min(int(n), k + 256), b, k) for b, n in enumerate(ns) for k in range(0, int(n), 256)], key=lambda x: -x[0])
        blk, n0, rows = np.array([x[1] for x in items], dtype=np.int32), np.array([x[2] for x in items], dtype=np.int32), None
    dev = [dv.f64(buf), dv.i64(pos[:-1]), dv.i32(lds), dv.i32(ns), dv.i32(off[:-1] if rows_per_real == 1 else [0]), dv.i32(blk), dv.i32(n0)]
    if rows is not None:
        dev.append(dv.i32(rows))
    keep.extend(dev)
    tp = lib.TdPlan()
    tp.Lbase = dev[0].data_ptr()
    tp.blk_pos, tp.blk_ld, tp.blk_n, tp.blk_off, tp.item_blk, tp.item_n0 = [x.data_ptr() for x in dev[1:7]]
    tp.item_rows = dev[7].data_ptr() if rows is not None else None
    tp.n_blocks, tp.n_items, tp.rows_per_real, tp.stream_kind, tp.rng_fast = len(Ls), len(blk), rows_per_real, kind, 0
    return tp, off


def _draw(gpu, Ls, rows_per_real, kind, M, zmem, partial_last):
    """pta_td_trmm_rng twice (bit-identical); returns the output and, with zmem, the deviates the device wrote and read"""
    lib, dv = gpu["lib"], gpu["dv"]
    keep = []
    tp, off = _plan(gpu, Ls, rows_per_real, kind, keep, partial_last)
    ns = [L.shape[0] for L in Ls]
    ntot = int(off[-1])
    z = None
    if zmem:
        if rows_per_real == 1:
            zoff = np.concatenate([[0], np.cumsum((np.array(ns) + 1) // 2 * 2)]).astype(np.int32)
            z = dv.zeros((M, int(zoff[-1]) + 16))
            keep += [dv.i32(ns), dv.i32(zoff[:-1])]
            lib.call("pta_rng_fill_normal_blocks", SEED, R0, M, kind, len(ns), dv.ptr(keep[-2]), dv.ptr(keep[-1]), int(max(ns)), dv.ptr(z), z.stride(0), 0, gpu["s"])
        else:       # row m = (realisation m // P, pulsar m % P): stream (kind, m % P), filled row by row
            P, n = rows_per_real, ns[0]
            npair = (n + 1) // 2
            z = dv.zeros((M, 2 * npair + 16))
            keep.append(dv.i32([0]))
            for m in range(M):
                lib.call("pta_rng_fill_normal", SEED, R0 + m // P, 1, philox_ref.stream_id(kind, m % P), npair, 1,
                         ctypes.c_void_p(z.data_ptr() + 8 * m * z.stride(0)), None, 2 * npair, 0, gpu["s"])
        tp.z, tp.ld_z, tp.blk_zoff = z.data_ptr(), z.stride(0), keep[-1].data_ptr()
    outs = []
    for rep in range(2):
        out = dv.f64(np.full((M, ntot + 3), 7.0))
        lib.call("pta_td_trmm_rng", ctypes.byref(tp), SEED, R0, M, dv.ptr(out), ntot + 3, gpu["s"])
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "second run differs"
    assert np.all(outs[0][:, ntot:] == 7.0)
    return outs[0], off, (z.cpu().numpy() if zmem else None)


def _draw_check(entry, got, L, z, drawn):
    ref, mag = tr.trmm_reference(L, z)
    assert np.all(np.isfinite(got))
    fill = tr.rho_c_rect(np.abs(got.astype(LD) - ref), tr.trmm_bound(mag, L.shape[0], drawn)) * U
    m = MEASURED.setdefault((entry, "draw"), [0.0, 0.0])
    m[0] = max(m[0], fill)
    assert fill <= 1.0, f"{entry}: n = {L.shape[0]} fills {fill:.3f} of its bound"


@pytest.mark.parametrize("partial_last", [False, True])
@pytest.mark.parametrize("zmem", [False, True])
@pytest.mark.parametrize("R", tc.DRAW_R)
def test_draw_per_pulsar_factors(gpu, R, zmem, partial_last):
    """pta_td_trmm_rng, rows_per_real = 1, on factors of Q and Lo: deviates from memory (the reference reads the same fp64 numbers) and
    generated in registers (the reference draws them in long double; 12 u per deviate), partial strip first and last"""
    Ls = _draw_factors()
    got, off, z = _draw(gpu, Ls, 1, 5, R, zmem, partial_last)
    zo = 0
    for b, L in enumerate(Ls):
        n = L.shape[0]
        zb = z[:, zo:zo + n] if zmem else np.stack([_drawn(5, b, m, n) for m in range(R)])
        zo += (n + 1) // 2 * 2
        _draw_check("draw memory" if zmem else "draw registers", got[:, off[b]:off[b] + n], L, zb, not zmem)


@pytest.mark.parametrize("zmem", [False, True])
@pytest.mark.parametrize("R", tc.DRAW_R[:2])
def test_draw_shared_factor(gpu, R, zmem):
    """rows_per_real = P: one factor (Lo, n = 513) for the rows (realisation, pulsar), stream (TDGW, pulsar)"""
    P, L = 3, _draw_factors()[-1]
    n = L.shape[0]
    got, _, z = _draw(gpu, [L], P, 6, R * P, zmem, False)
    zb = z[:, :n] if zmem else np.stack([_drawn(6, m % P, m // P, n) for m in range(R * P)])
    _draw_check("draw shared memory" if zmem else "draw shared registers", got[:, :n], L, zb, not zmem)


def test_report_measured_fractions():
    """the worst fraction of the bound per entry point and family of this session (pytest -s); nothing to assert beyond the cases'"""
    for (entry, fam), (fill, rn) in sorted(MEASURED.items()):
        print(f"MEASURED {entry:24s} {fam:5s} worst fraction {fill:.4f}  worst rho_n {rn:.1f}")
