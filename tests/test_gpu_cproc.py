"""Common red processes with an ORF of their own (add_common_process, theta's cp_* keys, red_noise.add_common_process) on the MI355X:
the coefficient kernel against the host twin and a long-double mix, the add kernel against the long-double synthesis of the device's
own coefficients, exact superposition on the engine without the processes, placement independence, theta and the prior draws, the
distribution of the coefficients, the discrimination of the injected ORFs by the correlated likelihood and the OS, and the refusals.

Bounds (u = 2^-53; cproc_reference.py):
  mix          |sum_j B z - exact| <= gamma_rho sum_j |B z|; a coefficient of n processes u sum_p (rho_p + n) amp_p sum_j |B_p z_p|
  add          8 n_f u sum_c |coef_c| per element (the issue's bound), plus u |result| for the one add of accumulate = 1
Measured on one MI355X (worst error / bound): coefficients 0.44 (bit-equal to the host twin); add 0.24 at n_f = 1, 0.14 at 2, 0.04 at 14
and 32; theta_r against the configured engine 1.2e-15; covariance entries within 2.3 standard errors; Lambda_monopole - Lambda_hd = +73.2
+- 0.97, Lambda_hd - Lambda_curn = +5.10 +- 0.09, mean OS SNR of a dipole injection 19.5 (dipole) against 3.8 (hd)."""
import ctypes

import numpy as np
import pytest
import torch

import cproc_reference as cr
from helpers import relrms

pytestmark = pytest.mark.gpu

TILE = 256
COUNTS = (TILE + 1, 1, TILE - 1, TILE, 2 * TILE + 3)   # tiles of 256, 1, 1, 255, 256, 256, 256 and 3 TOAs; tile starts on even and odd slots
FULL_COUNTS = (37, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
TOL_SIG = 1e-11   # tests/test_gpu_chrom.py's bound for an engine under theta_r against the configured one
_PSRS = {}


def _rg():
    from pta_replicator_amd import _lib
    return _lib.CPROC_RG


def _psrs(counts):
    if counts not in _PSRS:
        _PSRS[counts] = cr.make_psrs(counts)
    return _PSRS[counts]


def _user(P):
    return cr.rank2_orf(P)


def _engine(P=5, procs=(("monopole", 5, -13.6, 3.0), ("dipole", 3, -13.3, 2.0)), seed=77, full=False, counts=None):
    """white noise alone, or (full) + ECORR + red noise + GWB; orf "user" = the rank-2 array"""
    from pta_replicator_amd.engine import ReplicaEngine
    counts = counts or (FULL_COUNTS if full else COUNTS)
    eng = ReplicaEngine(_psrs(counts)[:P], seed=seed)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.1, log10_equad=-6.6)
    if full:
        eng.set_jitter(log10_ecorr=-6.7, coarsegrain=0.1)
        eng.set_red_noise([-14.0, -13.6, None, -13.9, -14.8][:P], [3.0, 2.2, None, 3.3, 1.5][:P], components=20)
        eng.set_gwb(-14.4, 13. / 3.)
    for orf, nf, lA, g in procs:
        eng.add_common_process(lA, g, orf=_user(P) if isinstance(orf, str) and orf == "user" else orf, components=nf)
    return eng


def _coef(eng, R, r0, lA=None, g=None):
    """coef [R, P, K] of pta_engine_cproc_coef alone, into a buffer of its own"""
    from pta_replicator_amd import _lib, device as dv
    c = eng._cproc_struct()
    coef = torch.full((R + 1, eng.P, c.k), -7.0, dtype=torch.float64, device="cuda")
    c.coef = coef.data_ptr()
    keep = []
    if lA is not None:
        lA_d, g_d = dv.f64(np.ascontiguousarray(lA)), dv.f64(np.ascontiguousarray(g))
        keep += [lA_d, g_d]
        c.log10_A, c.gamma = lA_d.data_ptr(), g_d.data_ptr()
    _lib.call("pta_engine_cproc_coef", ctypes.byref(c), eng.seed, r0, R, dv.stream_ptr())
    torch.cuda.synchronize()
    assert bool((coef[R] == -7.0).all())   # rows past R are untouched
    return coef[:R]


PROC_SETS = {
    1: (("hd", 1, -13.5, 3.0),),
    3: (("monopole", 2, -13.6, 3.0), ("dipole", 14, -13.3, 2.0), ("hd", 1, -13.9, 4.0)),
    5: (("monopole", 14, -13.6, 3.0), ("dipole", 32, -13.3, 2.0), ("curn", 2, -13.9, 4.0), ("user", 1, -13.7, 1.5)),
}


@pytest.mark.parametrize("P", [1, 3, 5])
def test_coefficients(P):
    """coef against the host twin on the same draws: with configured amplitudes bit for bit (the deviates are bit-equal, the sums the
    same fma chain); under theta to 16 u of the magnitudes (device pow / sqrt against libm's); against the long-double mix within the
    bound of the module docstring.  Ranks 1, 3, P and 2; processes of unequal components; R = 1, RG - 1, RG, RG + 1, 2 RG + 1."""
    RG = _rg()
    eng = _engine(P, PROC_SETS[P]).prepare()
    t = eng._cproc_t
    K, kp, Bs, n = t["K"], t["kp"], t["B_host"], len(t["kp"])
    assert t["rho"] == [[1], [1, 3, 3], [1, 3, 5, 2]][(P - 1) // 2]
    r0, Rmax = 2 ** 33 + 3, 2 * RG + 1
    full = _coef(eng, Rmax, r0).cpu().numpy()
    for R in (1, RG - 1, RG, RG + 1):
        assert np.array_equal(_coef(eng, R, r0).cpu().numpy(), full[:R]), R
    worst = 0.0
    for r in (0, RG, Rmax - 1):
        assert np.array_equal(full[r], cr.twin_coef(eng.seed, r0 + r, P, K, kp, Bs, t["amp_host"], t["T"])), r
        d = eng.dump_draws(r0 + r)["common"]
        for p in range(n):
            assert d[p].shape == (kp[p], Bs[p].shape[1]) and np.array_equal(d[p], cr.twin_draws(eng.seed, r0 + r, p, Bs[p].shape[1], kp[p])), (r, p)
            assert np.max(np.abs(d[p] - cr.draws(eng.seed, r0 + r, p, Bs[p].shape[1], kp[p]))) < 1e-13
        for c in range(K):
            val, bound = np.zeros(P, dtype=cr.LD), np.zeros(P)
            for p in range(n):
                if c < kp[p]:
                    v, mag = cr.mix_ld(Bs[p], d[p][c])
                    val += cr.LD(t["amp_host"][p, c]) * v
                    bound += cr.U * (Bs[p].shape[1] + n) * t["amp_host"][p, c] * mag
            err = np.abs(full[r, :, c].astype(cr.LD) - val)
            assert np.all(err <= bound), (r, c)
            worst = max(worst, float(np.max(err / bound)))
    print(f"P = {P}: worst |coef - long double| / bound = {worst:.3f}")
    rng = np.random.default_rng(P)
    lA, g = rng.uniform(-14.5, -13.0, (Rmax, n)), rng.uniform(1.0, 5.0, (Rmax, n))
    lA[0, 0] = np.nan
    lA[Rmax - 1] = np.nan
    got = _coef(eng, Rmax, r0, lA, g).cpu().numpy()
    assert np.array_equal(got[Rmax - 1], full[Rmax - 1])   # an all-NaN row is the configured one, bit for bit
    for r in (0, 1, RG + 1):
        want = cr.twin_coef(eng.seed, r0 + r, P, K, kp, Bs, t["amp_host"], t["T"], lA[r], g[r])
        mag = np.zeros((P, K))
        d = eng.dump_draws(r0 + r)["common"]
        for p in range(n):
            amp = t["amp_host"][p] if np.isnan(lA[r, p]) else np.concatenate([np.sqrt(cr.prior_phi(kp[p] // 2, t["T"], lA[r, p], g[r, p])),
                                                                               np.zeros(K - kp[p])])
            mag[:, :kp[p]] += amp[None, :kp[p]] * (np.abs(Bs[p]) @ np.abs(d[p]).T)
        assert np.all(np.abs(got[r] - want) <= 16 * cr.U * mag), r


@pytest.mark.parametrize("P,nf", [(1, 1), (1, 14), (3, 2), (3, 32), (5, 14), (5, 32), (5, 1)])
def test_add_against_long_double(P, nf):
    """pta_engine_cproc_add on the device's own coefficients against their long-double synthesis, for both accumulate modes, rows on
    even and odd 8-byte slots (a view at column 1 of a wider buffer, even and odd ld_out), R = 1, RG - 1, RG, RG + 1, 2 RG + 1; columns
    outside the tiles and rows past R keep their canary value"""
    RG = _rg()
    eng = _engine(P, (("hd", nf, -13.5, 3.0), ("monopole", max(1, nf // 2), -13.2, 2.0))).prepare()
    t, n = eng._cproc_t, eng.n_toa
    toas = np.concatenate(eng._cproc_toas())
    Rmax = 2 * RG + 1
    coef = _coef(eng, Rmax, 5).contiguous()
    ch = coef.cpu().numpy()
    F = cr.basis_ld(toas, t["T"], nf)
    val = np.empty((Rmax, n), dtype=cr.LD)
    bound = np.empty((Rmax, n))
    for a in range(P):
        sl = slice(eng.off[a], eng.off[a + 1])
        val[:, sl] = ch[:, a, :].astype(cr.LD) @ F[sl].T
        bound[:, sl] = (8 * nf * cr.U * np.sum(np.abs(ch[:, a, :]), axis=1))[:, None]
    worst = 0.0
    prev = torch.as_tensor(np.random.default_rng(nf).normal(size=(Rmax, n)) * 1e-6, device="cuda")
    first = eng._cproc_add_coef(coef, Rmax, torch.full((Rmax, n), -7.0, dtype=torch.float64, device="cuda")).cpu().numpy()
    for R in (1, RG - 1, RG, RG + 1, Rmax):
        for pad, col in ((2, 0), (4, 1), (5, 1), (3, 0)):   # aligned rows; every row odd; rows alternating (odd ld_out), from odd and even starts
            for acc in (False, True):
                wide = torch.full((R + 2, n + pad), -7.0, dtype=torch.float64, device="cuda")
                view = wide[1:R + 1, col:col + n]
                if acc:
                    view.copy_(prev[:R])
                eng._cproc_add_coef(coef[:R], R, view, accumulate=acc)
                torch.cuda.synchronize()
                w = wide.cpu().numpy()
                assert np.all(w[0] == -7.0) and np.all(w[R + 1] == -7.0) and np.all(w[:, :col] == -7.0) and np.all(w[:, col + n:] == -7.0)
                got = w[1:R + 1, col:col + n]
                if acc:
                    want = val[:R] + prev[:R].cpu().numpy().astype(cr.LD)
                    # |fl(prev + t~) - (prev + t)| <= |t~ - t| + u |prev + t~| <= b + u (|prev + t| + b)
                    lim = bound[:R] * (1 + cr.U) + cr.U * np.abs(want).astype(np.float64)
                else:
                    want, lim = val[:R], bound[:R]
                    assert np.array_equal(got, first[:R])   # the same bits in every slot, alignment and batch
                err = np.abs(got.astype(cr.LD) - want).astype(np.float64)
                assert np.all(err <= lim), (R, pad, col, acc, float(np.max(err / lim)))
                if not acc:
                    worst = max(worst, float(np.max(err / lim)))
    # and the kernel's loop is the host twin's, bit for bit
    sc1 = t["sc1_host"]
    for a in range(P):
        sl = slice(eng.off[a], eng.off[a + 1])
        assert np.array_equal(first[0, sl], cr.twin_synth(ch[0, a], sc1[sl]))
    print(f"P = {P}, n_f = {nf}: worst |add - long double| / bound = {worst:.3f}")


def test_unchanged_engine():
    """an engine without add_common_process is what it was: no tables, no 'common' entry or draws, and rows that do not depend on how they
    are batched - the checks the engine passed before the method existed"""
    eng = _engine(procs=(), full=True).prepare()
    assert not getattr(eng, "_cproc", None) and getattr(eng, "_cproc_t", None) is None
    sig = eng.generate_per_signal(5, r0=3)
    assert set(sig) == {"total", "rn", "gwb", "wn", "ecorr"} and set(eng.dump_draws(3)) == {"gwb", "rn", "wn", "ecorr"}
    rows = eng.generate(5, r0=3)
    assert torch.equal(rows, sig["total"])
    assert torch.equal(torch.cat([eng.generate(1, r0=3 + r) for r in range(5)]), rows)


def test_exact_superposition_per_signal_and_replay():
    """generate of the engine = generate of the engine without the processes + generate_per_signal()["common"], one fp64 add per element;
    every other per-signal entry is the one of the engine without them; with theta of both kinds too; replay(dump_draws(r)) reproduces
    the row to the bound of the existing replay tests, and its 'common' entry the device's to the add kernel's bound"""
    RG = _rg()
    R, r0 = 2 * RG + 1, 11
    procs = (("monopole", 5, -13.6, 3.0), ("dipole", 3, -13.3, 2.0), ("user", 7, -13.5, 2.5))
    with_c, without = _engine(procs=procs, full=True).prepare(), _engine(procs=(), full=True).prepare()
    sig, sig0 = with_c.generate_per_signal(R, r0=r0), without.generate_per_signal(R, r0=r0)
    assert set(sig) == set(sig0) | {"common"}
    for k in sig0:
        if k != "total":
            assert torch.equal(sig[k], sig0[k]), k
    assert torch.equal(with_c.generate(R, r0=r0), without.generate(R, r0=r0) + sig["common"])
    assert torch.equal(sig["total"], sig0["total"] + sig["common"])
    assert float(sig["common"].abs().max()) > 0
    rng = np.random.default_rng(2)
    P = with_c.P
    other = dict(rn_log10_A=rng.uniform(-15, -13, (R, P)), rn_gamma=rng.uniform(1, 5, (R, P)), gwb_log10_A=rng.uniform(-15, -14, R),
                 gwb_gamma=rng.uniform(3, 5, R), wn_efac=rng.uniform(0.5, 2.0, (R, P)))
    th = dict(cp_log10_A=rng.uniform(-14.5, -13.0, (R, 3)), cp_gamma=rng.uniform(1.0, 5.0, (R, 3)))
    term = with_c.generate_per_signal(R, r0=r0, theta=th)["common"]
    assert not torch.equal(term, sig["common"])
    assert torch.equal(with_c.generate(R, r0=r0, theta=dict(other, **th)), without.generate(R, r0=r0, theta=other) + term)
    out = with_c.generate(4, r0=5).cpu().numpy()
    common = with_c.generate_per_signal(4, r0=5)["common"].cpu().numpy()
    for r in (0, 3):
        d = with_c.dump_draws(5 + r)
        assert set(d) == {"gwb", "rn", "wn", "ecorr", "common"} and len(d["common"]) == 3
        rep = with_c.replay([d], per_signal=True)
        tot = rep["total"].cpu().numpy()[0]
        assert np.max(np.abs(out[r] - tot)) < 1e-12 * np.sqrt(np.mean(tot ** 2))
        assert torch.equal(rep["total"], ((((rep["rn"] + rep["common"]) + rep["gwb"]) + rep["wn"]) + rep["ecorr"]))
        got = rep["common"].cpu().numpy()[0]
        for a in range(P):   # the host's B @ z against the device's fma chain: a few u of the coefficients, through a basis of unit size
            sl = slice(with_c.off[a], with_c.off[a + 1])
            assert relrms(got[sl], common[r, sl]) < 1e-13


def test_single_pulsar_without_gwb_and_list_api():
    """P = 1 without set_gwb: every ORF is the number 1, the term superposes exactly.  The list twin: the legacy deviates (column major,
    factor column minor) mixed on the host and synthesised by the same add kernel - equal to the engine's add kernel on the same mix, bit
    for bit - recorded under added_signals"""
    from pta_replicator_amd.red_noise import add_common_process
    one, plain = _engine(1, (("hd", 3, -13.5, 3.0), ("monopole", 2, -13.8, 2.0))).prepare(), _engine(1, ()).prepare()
    term = one.generate_per_signal(3, r0=1)["common"]
    assert torch.equal(one.generate(3, r0=1), plain.generate(3, r0=1) + term) and float(term.abs().max()) > 0
    from pta_replicator_amd import device as dv
    from pta_replicator_amd.engine import ReplicaEngine
    psrs = cr.make_psrs(COUNTS[:3], seed=5)
    eng = ReplicaEngine(psrs, seed=1)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.add_common_process(-13.4, 2.7, orf="dipole", components=4)
    eng.prepare()
    np.random.seed(1234)
    z = np.random.randn(8 * 3).reshape(8, 3)
    coef = eng._cproc_t["amp_host"][0][None, :] * (eng._cproc_t["B_host"][0] @ z.T)
    want = eng._cproc_add_coef(dv.f64(coef[None]), 1, dv.zeros((1, eng.n_toa))).cpu().numpy()[0]
    add_common_process(psrs, -13.4, 2.7, orf="dipole", components=4, seed=1234)
    for a, p in enumerate(psrs):
        got = np.asarray(p.added_signals_time[f"{p.name}_common_process"].value)
        assert np.array_equal(got, want[eng.off[a]:eng.off[a + 1]]) and np.any(got != 0)
        assert p.added_signals[f"{p.name}_common_process"] == {"amplitude": -13.4, "spectral_index": 2.7, "orf": "dipole", "components": 4}


def test_batch_independence():
    """a row is the same bits in one call, in calls of one, at another r0 slot, in several batches (max_batch), inside generate_os whatever
    the chunk, and when out is a view at an odd column of a wider buffer with odd ld_out, whose other columns stay untouched"""
    RG = _rg()
    R, r0 = 2 * RG + 3, 70
    rng = np.random.default_rng(21)
    th = dict(cp_log10_A=rng.uniform(-14.5, -13.0, (R, 2)), cp_gamma=rng.uniform(1.0, 5.0, (R, 2)))
    th["cp_log10_A"][R - 1] = np.nan
    eng = _engine(full=True).prepare()
    full = eng.generate(R, r0=r0, theta=th)
    for r in (0, RG - 1, RG, R - 1):
        assert torch.equal(eng.generate(1, r0=r0 + r, theta={k: v[r:r + 1] for k, v in th.items()})[0], full[r]), r
    assert torch.equal(eng.generate(R - 5, r0=r0 + 5, theta={k: v[5:] for k, v in th.items()}), full[5:])
    small = _engine(full=True)
    small.workspace_bytes = 1
    small.prepare()
    assert small.max_batch() < R
    assert torch.equal(small.generate(R, r0=r0, theta=th), full)
    n = eng.n_toa
    for pad in (4, 5):   # even and odd ld_out: every row on an odd 8-byte slot, then rows alternating
        wide = torch.full((R, n + pad), -7.0, dtype=torch.float64, device="cuda")
        view = wide[:, 1:1 + n]
        assert eng.generate(R, r0=r0, out=view, theta=th) is view
        assert torch.equal(view, full)
        assert bool((wide[:, :1] == -7.0).all()) and bool((wide[:, 1 + n:] == -7.0).all())
    eng.prepare_optimal_statistic(components=6)
    want = eng.optimal_statistic(full)["A2"]
    for chunk in (1, 7, RG + 1, R):
        assert torch.equal(eng.generate_os(R, r0=r0, theta=th, chunk=chunk)["A2"], want), chunk
    host = np.concatenate([x.copy() for _, x in eng.stream_to_host(R, chunk=RG + 1, r0=r0)])
    assert np.array_equal(host, eng.generate(R, r0=r0).cpu().numpy())


def test_theta_and_prior():
    """an all-NaN cp_log10_A equals no theta bit for bit; a row under theta_r equals an engine configured with theta_r to TOL_SIG; a key
    given alone keeps the other parameter; generate_sampled labels lie inside their boxes, are philox_ref's map of stream (7, 8) and (7, 9),
    do not depend on the batch, and leave every pre-existing label bit-identical"""
    from pta_replicator_amd import _cproc
    procs = (("monopole", 5, -13.6, 3.0), ("hd", 3, -13.3, 2.0))
    eng = _engine(procs=procs).prepare()
    R, r0 = 4, 9
    base = eng.generate_per_signal(R, r0=r0)["common"]
    nan = dict(cp_log10_A=np.full((R, 2), np.nan), cp_gamma=np.full((R, 2), np.nan))
    assert torch.equal(eng.generate_per_signal(R, r0=r0, theta=nan)["common"], base)
    assert torch.equal(eng.generate(R, r0=r0, theta=nan), eng.generate(R, r0=r0))
    rng = np.random.default_rng(8)
    th = dict(cp_log10_A=rng.uniform(-14.5, -13.0, (R, 2)), cp_gamma=rng.uniform(1.0, 5.0, (R, 2)))
    got = eng.generate_per_signal(R, r0=r0, theta=th)["common"].cpu().numpy()
    only_A = eng.generate_per_signal(R, r0=r0, theta={"cp_log10_A": th["cp_log10_A"]})["common"].cpu().numpy()
    only_g = eng.generate_per_signal(R, r0=r0, theta={"cp_gamma": th["cp_gamma"]})["common"].cpu().numpy()
    worst = 0.0
    for r in range(R):
        for key, have in (("both", got), ("A", only_A), ("g", only_g)):
            lA = th["cp_log10_A"][r] if key != "g" else [-13.6, -13.3]
            g = th["cp_gamma"][r] if key != "A" else [3.0, 2.0]
            conf = _engine(procs=tuple((o, nf, float(lA[i]), float(g[i])) for i, (o, nf, _, _) in enumerate(procs))).prepare()
            want = conf.generate_per_signal(1, r0=r0 + r)["common"].cpu().numpy()[0]
            for a in range(eng.P):
                sl = slice(eng.off[a], eng.off[a + 1])
                worst = max(worst, relrms(have[r, sl], want[sl]))
    print(f"theta_r against the engine configured with theta_r: worst per-pulsar relative RMS deviation = {worst:.2e}")
    assert worst < TOL_SIG
    full = _engine(procs=procs, full=True).prepare()
    R, r0 = 7, 40
    other = dict(gwb_log10_A=(-15, -13), gwb_gamma=(3, 5), rn_log10_A=(-15, -13), rn_gamma=(1, 5), wn_efac=(0.5, 2.0))
    full.set_hyper_prior(**other)
    a, tha = full.generate_sampled(R, r0=r0)
    boxes = dict(cp_log10_A=(-14.5, -13.0), cp_gamma=np.array([[1.0, 2.0], [3.0, 5.0]]))
    full.set_hyper_prior(**other, **boxes)
    b, thb = full.generate_sampled(R, r0=r0)
    assert set(thb) == set(tha) | set(_cproc.KEYS)
    for k in tha:
        assert np.array_equal(tha[k].cpu().numpy(), thb[k].cpu().numpy(), equal_nan=True), k
    assert not torch.equal(a, b)
    from oracle import philox_ref as ph
    for k, field in (("cp_log10_A", cr.FIELD_LOG10_A), ("cp_gamma", cr.FIELD_GAMMA)):
        lo, hi = (np.broadcast_to(np.asarray(boxes[k], dtype=float), (2, 2))[:, j] for j in (0, 1))
        lab = thb[k].cpu().numpy()
        assert lab.shape == (R, 2) and np.all(lab >= lo) and np.all(lab <= hi)
        for r in range(R):
            _, u2 = ph.uniform_pairs(full.seed, r0 + r, ph.stream_id(7, field), 2)
            want = lo + (hi - lo) * np.asarray(u2)
            assert np.all(np.abs(lab[r] - want) <= np.spacing(np.abs(want))), (k, r)
    assert torch.equal(full.generate(R, r0=r0, theta={k: torch.as_tensor(v.cpu().numpy()) for k, v in thb.items()}), b)
    c, thc = full.generate_sampled(1, r0=r0 + 3)
    assert torch.equal(c[0], b[3]) and all(torch.equal(thc[k][0], thb[k][3]) for k in _cproc.KEYS)
    full.set_hyper_prior(**boxes)   # common-process boxes alone are a prior
    d, thd = full.generate_sampled(R, r0=r0)
    assert set(thd) == set(_cproc.KEYS) and all(torch.equal(thd[k], thb[k]) for k in thd)
    assert torch.equal(d, full.generate(R, r0=r0, theta=thd))


@pytest.mark.parametrize("orf", ["hd", "monopole", "dipole", "curn"])
def test_distribution(orf):
    """P = 5, n_f = 2, R = 4096: the sample covariance of coef between pulsars against phi_c Gamma_ab, every one of the 60 entries (15
    pairs a <= b x 4 columns) within 5 of its own standard error phi_c sqrt((1 + Gamma_ab^2) / R) (Wishart, unit diagonal); fixed seed"""
    P, R = 5, 4096
    eng = _engine(P, ((orf, 2, -13.5, 3.0),), seed=2024).prepare()
    y = _coef(eng, R, 0).cpu().numpy()
    Gamma, phi = eng._cproc[0]["Gamma"], eng._cproc_t["amp_host"][0] ** 2
    assert np.allclose(np.diag(Gamma), 1.0)
    worst, count = 0.0, 0
    for c in range(4):
        cov = y[:, :, c].T @ y[:, :, c] / R
        for a in range(P):
            for b in range(a, P):
                se = phi[c] * np.sqrt((1 + Gamma[a, b] ** 2) / R)
                worst = max(worst, abs(cov[a, b] - phi[c] * Gamma[a, b]) / se)
                count += 1
    print(f"{orf}: worst |cov - phi Gamma| = {worst:.2f} standard errors over {count} entries")
    assert count == 60 and worst < 5.0


def _clnl_engine(orf):
    """the setting of tests/test_gpu_clnl.py's discrimination check: 16 pulsars, 0.1 us white noise, n_f = 5; no set_gwb"""
    from pta_replicator_amd.engine import ReplicaEngine
    from test_gpu_os import _psrs as os_psrs
    eng = ReplicaEngine(os_psrs(16, 200, 21, step=0, sessions=False, err_us=0.1), seed=8)
    eng.td_warmup = False
    eng.set_white_noise(efac=1.0)
    eng.add_common_process(-14.0, 13. / 3., orf=orf, components=5)
    return eng.prepare()


@pytest.mark.parametrize("orf,other", [("monopole", "hd"), ("hd", "curn")])
def test_discrimination_by_the_correlated_likelihood(orf, other):
    """a monopole process at log10_A = -14 gives Lambda_monopole - Lambda_hd > 0, and an "hd" process without set_gwb Lambda_hd -
    Lambda_curn > 0, by more than 5 standard errors of the mean over R = 256 in generate_correlated_lnl at the injected (A, gamma)"""
    eng = _clnl_engine(orf)
    eng.prepare_correlated_likelihood(components=5, orfs=(orf, other))
    R = 256
    lam = eng.generate_correlated_lnl(R, {"gwb_log10_A": np.array([-14.0])})["lnl_ratio"][:, :, 0].cpu().numpy()
    d = lam[:, 0] - lam[:, 1]
    mean, se = float(d.mean()), float(d.std(ddof=1) / np.sqrt(R))
    print(f"{orf} injection: mean Lambda_{orf} - Lambda_{other} = {mean:.3f} +- {se:.3f} ({mean / se:.1f} standard errors)")
    assert np.all(np.isfinite(lam)) and mean > 5 * se


def test_dipole_in_the_optimal_statistic():
    """a dipole injection gives a mean dipole SNR from generate_os above the HD SNR of the same rows"""
    eng = _clnl_engine("dipole")
    eng.prepare_optimal_statistic(components=5, orfs=("hd", "monopole", "dipole"), gwb_auto=False)
    snr = eng.generate_os(256)["snr"].cpu().numpy()
    mean = snr.mean(axis=0)
    print(f"dipole injection: mean OS SNR hd {mean[0]:.2f}, monopole {mean[1]:.2f}, dipole {mean[2]:.2f}")
    assert snr.shape == (256, 3) and mean[2] > mean[0]


def test_refusals_on_the_device_path():
    """on a prepared engine: TD mode, the likelihood, the matched OS, cp_* on a likelihood grid, a fifth process, a non-PSD user ORF,
    components = 33 - each a ValueError that names the reason; the prepared engine keeps generating"""
    procs = (("monopole", 2, -13.6, 3.0), ("dipole", 2, -13.3, 2.0), ("hd", 2, -13.3, 2.0), ("curn", 2, -13.3, 2.0))
    eng = _engine(procs=procs, full=True).prepare()
    before = eng.generate(2)
    R = 3
    for call in (lambda: eng.generate_td(R), lambda: eng.prepare_td(), lambda: eng.generate_os(R, td=True)):
        with pytest.raises(ValueError, match="common process.*no TD mode"):
            call()
    with pytest.raises(ValueError, match="prepare_likelihood.*common process"):
        eng.prepare_likelihood()
    with pytest.raises(ValueError, match=r"matched=True.*common process"):
        eng.prepare_optimal_statistic(matched=True)
    eng.prepare_correlated_likelihood(components=3, orfs=("hd", "monopole"))
    for grid in ({"cp_log10_A": np.full(2, -14.0)}, {"gwb_log10_A": np.full(2, -14.0), "cp_gamma": np.full(2, 3.0)}):
        with pytest.raises(ValueError, match="cp_"):
            eng.generate_correlated_lnl(R, grid)
        with pytest.raises(ValueError, match="cp_"):
            eng.correlated_log_likelihood(before, grid)
    with pytest.raises(ValueError, match="at most 4 common processes"):
        eng.add_common_process(-14.0, 3.0)
    bad = np.eye(eng.P)
    bad[0, 1] = bad[1, 0] = 2.0
    three = _engine(procs=procs[:3]).prepare()
    with pytest.raises(ValueError, match="not positive semi-definite"):
        three.add_common_process(-14.0, 3.0, orf=bad)
    with pytest.raises(ValueError, match="components"):
        three.add_common_process(-14.0, 3.0, components=33)
    assert three._prepared and len(three._cproc) == 3
    assert torch.equal(eng.generate(2), before)
