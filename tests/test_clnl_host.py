"""Host half of the correlated likelihood ratio (optimal_statistic.py: orf_matrix, orf_factor, clnl_plan, clnl_scale, clnl_from_rows)
against a dense likelihood built here - explicit C_a, the timing model removed by projecting on its null space, np.kron(Gamma, diag phi) -
the two forms of the NumPy twin against each other, "curn" against the uncorrelated likelihood (lnl_from_rows), the ORF factors,
csrc/pta_clnl.h compiled with g++ against clnl_scale, and the refusals.  No GPU.

Bound of the dense comparison: |fast - dense| / (|Lambda| + 1) < 1e-9 over the whole 3 x 3 grid of log10_A in {-15.5, -14, -13} and gamma in
{3, 13/3, 6}, with the dense likelihoods evaluated in long double (a float64 dense form is itself at 2e-9 at (-13, 6), and at 4e-9 at
log10_A = -12, which is not part of the check).  Measured: 2.2e-11 at the most (the two forms of the twin: 3.5e-13)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pta_replicator_amd import optimal_statistic as ost
from pta_replicator_amd.constants import YEAR_IN_SEC
from pta_replicator_amd.simulate import timing_design_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
P, NF, GREF = 5, 3, 13. / 3.
COUNTS = [37, 52, 41, 64, 45]
LOG10_A = (-15.5, -14.0, -13.0)
GAMMAS = (3.0, 13. / 3., 6.0)
GRID_A, GRID_G = [np.ravel(x) for x in np.meshgrid(LOG10_A, GAMMAS, indexing="ij")]
KRN = 4


def _array():
    """5 ragged pulsars of 37 .. 64 TOAs: ECORR epochs of three TOAs, red noise on 4 frequencies of the pulsar's own span"""
    rng = np.random.default_rng(3)
    t0, span = 53000 * 86400.0, 10 * YEAR_IN_SEC
    arr = dict(toas=[np.sort(t0 + rng.uniform(0, span * rng.uniform(0.6, 1.0), n)) for n in COUNTS])
    arr["sigma2"] = [rng.uniform(0.5e-7, 3e-7, n) ** 2 for n in COUNTS]
    pos = rng.normal(size=(P, 3))
    arr["pos"] = pos / np.linalg.norm(pos, axis=1)[:, None]
    arr["epoch_of"] = [np.arange(n) // 3 for n in COUNTS]
    arr["ecorr"] = [np.full(e.max() + 1, 2e-7) for e in arr["epoch_of"]]
    arr["F_rn"], arr["phi_rn"] = [], []
    for t in arr["toas"]:
        T = t.max() - t.min()
        f = np.arange(1, KRN + 1) / T
        a = 2 * np.pi * t[:, None] * f[None, :]
        F = np.empty((len(t), 2 * KRN))
        F[:, 0::2], F[:, 1::2] = np.sin(a), np.cos(a)
        arr["F_rn"].append(F)
        arr["phi_rn"].append((10 ** -13.5) ** 2 * (np.repeat(f, 2) * YEAR_IN_SEC) ** (-3.5) / (12 * np.pi ** 2 * T) * YEAR_IN_SEC ** 3)
    rows = np.concatenate([rng.normal(0, np.sqrt(s2) * 3, (7, len(s2))) for s2 in arr["sigma2"]], axis=1)
    arr["rows"] = rows + 3e-7 * np.sin(2 * np.pi * np.concatenate(arr["toas"]) / span)[None, :] * rng.normal(size=(7, 1))
    return arr


ARR = _array()


def _M(model):
    return None if model is None else [timing_design_matrix(t, model=model)[0] for t in ARR["toas"]]


def _user_orf():
    rng = np.random.default_rng(8)
    A = rng.normal(size=(P, 3))
    G = A @ A.T + 0.3 * np.eye(P)                       # positive definite, not unit diagonal: used as given
    return 0.5 * (G + G.T)


def _plan(with_ecorr, model, rn=True):
    return ost.prepare(ARR["toas"], ARR["sigma2"], ARR["pos"], components=NF, gamma=GREF, orfs=("hd",), epoch_of=ARR["epoch_of"] if with_ecorr else None,
                       ecorr=ARR["ecorr"] if with_ecorr else None, F_rn=ARR["F_rn"] if rn else None, phi_rn=ARR["phi_rn"] if rn else None, gw_amp2=0.0,
                       M=_M(model))


LD = np.longdouble


def _chol_ld(A):
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _ln_ld(Cm, rp):
    """-1/2 r^T C^-1 r - 1/2 ln det C of the columns of rp, in long double"""
    L = _chol_ld(Cm)
    z = rp.copy()
    for i in range(len(L)):
        z[i] = (z[i] - L[i, :i] @ z[:i]) / L[i, i]
    return -0.5 * np.sum(z * z, axis=0) - np.sum(np.log(np.diag(L)))


class _Dense:
    """ln L(r | common process) - ln L(r | noise only) of ARR's rows through dense matrices over all TOAs of the array: explicit C_a, the
    timing model removed by projecting on its null space (the left singular vectors beyond its columns), np.kron(Gamma, diag phi).  The
    matrices are built in float64 and the two likelihoods evaluated in long double: in float64 this form is itself off by 2e-9 at
    (log10_A, gamma) = (-13, 6), where eig(M) reaches 2.6e3 (against long double there: the fast form 1.1e-12, this form 2.1e-9)."""

    def __init__(self, plan, with_ecorr, model):
        N, C = sum(COUNTS), 2 * NF
        off = np.concatenate([[0], np.cumsum(COUNTS)])
        Cn, Fb, Gs = np.zeros((N, N)), np.zeros((N, P * C)), []
        M = _M(model)
        for a in range(P):
            s = slice(off[a], off[a + 1])
            Ca = np.diag(ARR["sigma2"][a]) + ARR["F_rn"][a] @ np.diag(ARR["phi_rn"][a]) @ ARR["F_rn"][a].T
            if with_ecorr:
                E = np.zeros((COUNTS[a], ARR["epoch_of"][a].max() + 1))
                E[np.arange(COUNTS[a]), ARR["epoch_of"][a]] = 1
                Ca = Ca + E @ np.diag(ARR["ecorr"][a] ** 2) @ E.T
            Cn[s, s] = Ca
            Fb[s, a * C:(a + 1) * C] = ost.fourier_basis(ARR["toas"][a], NF, plan.T)
            Gs.append(np.eye(COUNTS[a]) if M is None else np.linalg.svd(M[a])[0][:, M[a].shape[1]:])
        Gn = np.zeros((N, sum(x.shape[1] for x in Gs)))
        c = 0
        for a in range(P):
            Gn[off[a]:off[a + 1], c:c + Gs[a].shape[1]] = Gs[a]
            c += Gs[a].shape[1]
        self.sc = float(np.mean(np.diag(Cn)))
        Gl = Gn.astype(LD)
        self.C0 = Gl.T @ (Cn / self.sc).astype(LD) @ Gl
        self.GF = Gl.T @ Fb.astype(LD)
        self.rp = ((ARR["rows"].astype(LD) @ Gl) / np.sqrt(LD(self.sc))).T.copy()
        self.ln0 = _ln_ld(self.C0, self.rp)
        self.T = plan.T

    def __call__(self, Gamma, lA, g):
        Phi = (np.kron(Gamma, np.diag(10 ** (2 * lA) * ost.unit_spectrum(NF, self.T, g))) / self.sc).astype(LD)
        return (_ln_ld(self.C0 + self.GF @ Phi @ self.GF.T, self.rp) - self.ln0).astype(np.float64)


@pytest.mark.parametrize("model", ["spin", None])
@pytest.mark.parametrize("with_ecorr", [True, False])
def test_clnl_vs_dense(with_ecorr, model):
    plan = _plan(with_ecorr, model)
    cp = ost.clnl_plan(plan, ("hd", "monopole", "dipole", "curn"), gamma_ref=GREF)
    cu = ost.clnl_plan(plan, (_user_orf(),), gamma_ref=GREF)
    assert cp.rho == [5, 1, 3, 5] and cu.rho == [5] and cp.names == ["hd", "monopole", "dipole", "curn"] and cu.names == ["orf0"]
    worst = worst_forms = 0.0
    dense_of = _Dense(plan, with_ecorr, model)
    for c in (cp, cu):
        fast = ost.clnl_from_rows(c, ARR["rows"], GRID_A, GRID_G)
        alt = ost.clnl_from_rows(c, ARR["rows"], GRID_A, GRID_G, form="solve")
        assert fast.shape == (7, len(c.names), 9)
        Y = ost.project(plan, ARR["rows"])
        d = ost.clnl_scale(NF, plan.T, GREF, GRID_A, GRID_G)
        for o in range(len(c.names)):
            B = c.B[o]
            Yp = np.einsum("ai,rac->ric", B, Y).reshape(7, -1)
            for k in range(9):
                dense = dense_of(c.Gamma[o], GRID_A[k], GRID_G[k])
                worst = max(worst, float(np.max(np.abs(fast[:, o, k] - dense) / (np.abs(dense) + 1))))
                D = np.tile(d[k], B.shape[1])
                Mg = np.eye(len(D)) + D[:, None] * c.T_orf[o] * D[None, :]
                assert np.linalg.eigvalsh(Mg)[0] >= 1 - 1e-12
                scale = 0.5 * np.sum((D[None, :] * Yp) ** 2, axis=1) + abs(np.linalg.slogdet(Mg)[1])
                worst_forms = max(worst_forms, float(np.max(np.abs(fast[:, o, k] - alt[:, o, k]) / scale)))
    print(f"ecorr={with_ecorr} model={model}: worst |fast - dense| / (|Lambda| + 1) {worst:.2e}, the two forms {worst_forms:.2e}")
    assert worst < 1e-9
    assert worst_forms < 1e-8


def test_curn_is_the_uncorrelated_likelihood():
    """Gamma = I: the ratio is the sum over pulsars of ln L(grid point) - ln L(vanishing amplitude) of the uncorrelated likelihood, on
    a noise model without red noise (lnl_from_rows would put red-noise columns on the grid; here its grid holds the common process alone)"""
    plan = _plan(True, "spin", rn=False)
    cp = ost.clnl_plan(plan, ("curn",), gamma_ref=GREF)
    fast = ost.clnl_from_rows(cp, ARR["rows"], GRID_A, GRID_G)[:, 0, :]
    lp = ost.prepare_lnl(ARR["toas"], ARR["sigma2"], components=NF, epoch_of=ARR["epoch_of"], ecorr=ARR["ecorr"], M=_M("spin"))
    G = len(GRID_A)
    b = ost.matched_prior(G, lp.s, nf=NF, T=lp.T, gw_log10_A=GRID_A, gw_gamma=GRID_G)
    b0 = ost.matched_prior(1, lp.s, nf=NF, T=lp.T, gw_log10_A=np.array([-30.0]), gw_gamma=np.array([GREF]))
    ref = ost.lnl_from_rows(lp, ARR["rows"], b)[1] - ost.lnl_from_rows(lp, ARR["rows"], b0)[1]
    worst = float(np.max(np.abs(fast - ref) / (np.abs(ref) + 1)))
    print(f"curn against lnl_from_rows: worst {worst:.2e}")
    assert worst < 1e-9


def test_orf_matrix_and_factor():
    pos = ARR["pos"]
    pa, pb, cz = ost.pair_geometry(pos)
    hd = ost.orf_matrix("hd", pos)
    assert np.array_equal(np.diag(hd), np.ones(P)) and np.array_equal(hd, hd.T) and np.array_equal(hd[pa, pb], ost.hd(cz))
    assert np.array_equal(ost.orf_matrix("curn", pos), np.eye(P)) and np.array_equal(ost.orf_matrix("monopole", pos), np.ones((P, P)))
    assert np.array_equal(ost.orf_matrix("dipole", pos)[pa, pb], cz)
    U = _user_orf()
    assert np.array_equal(ost.orf_matrix(U, pos), U)
    for name, rank in (("monopole", 1), ("dipole", 3), ("hd", P), ("curn", P)):
        G = ost.orf_matrix(name, pos)
        B = ost.orf_factor(G)
        assert B.shape == (P, rank), name
        assert np.max(np.abs(B @ B.T - G)) < 1e-14, name
    assert ost.orf_factor(np.ones((1, 1))).shape == (1, 1)
    Q = np.linalg.qr(np.random.default_rng(1).normal(size=(P, P)))[0]
    bad = (Q * np.array([1.0, 0.8, 0.5, 0.2, -1e-3])) @ Q.T
    with pytest.raises(ValueError, match="positive semi-definite"):
        ost.orf_factor(0.5 * (bad + bad.T))
    with pytest.raises(ValueError, match="rank 0"):
        ost.orf_factor(np.zeros((P, P)))
    with pytest.raises(ValueError, match="symmetric"):
        ost.orf_factor(np.triu(np.ones((P, P))))
    with pytest.raises(ValueError, match="symmetric"):
        ost.orf_matrix(np.triu(np.ones((P, P))), pos)
    with pytest.raises(ValueError, match="unknown ORF"):
        ost.orf_matrix("quadrupole", pos)
    with pytest.raises(ValueError, match="1 .. 4"):
        ost.clnl_plan(_plan(False, None), ("hd",) * 5)


# ---------------------------------------------------------------- device math header ----------------------------------------
@pytest.fixture(scope="module")
def ch(tmp_path_factory):
    out = tmp_path_factory.mktemp("clnl") / "libclnlhost.so"
    src = os.path.join(HERE, "clnl", "clnl_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", str(out)])
    lib = ctypes.CDLL(str(out))
    i, d, pd = ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    lib.ch_scale.argtypes = [i, d, d, pd, pd, i, pd]
    lib.ch_scale.restype = None
    lib.ch_m_entry.argtypes = [d, d, d, i]
    lib.ch_m_entry.restype = d
    lib.ch_value.argtypes = [d, d]
    lib.ch_value.restype = d
    return lib


def test_scale_header_matches_numpy(ch):
    T = float(_plan(False, None).T)
    pd = ctypes.POINTER(ctypes.c_double)
    for nf in (NF, 14):
        ref = ost.clnl_scale(nf, T, GREF, GRID_A, GRID_G)
        got = np.full_like(ref, np.nan)
        ch.ch_scale(2 * nf, T, GREF, GRID_A.ctypes.data_as(pd), GRID_G.ctypes.data_as(pd), len(GRID_A), got.ctypes.data_as(pd))
        ulp = float(np.max(np.abs(got - ref) / np.spacing(ref)))
        print(f"n_f = {nf}: clnl_scale against pta_clnl_scale, worst {ulp:.1f} ulp")
        assert ulp <= 2
    # d^2 = phi_g / S_ref: the grid point's spectrum over the unit spectrum of the plan
    phi = 10 ** (2 * GRID_A[:, None]) * np.stack([ost.unit_spectrum(NF, T, g) for g in GRID_G])
    assert np.max(np.abs(ost.clnl_scale(NF, T, GREF, GRID_A, GRID_G) ** 2 / (phi / ost.unit_spectrum(NF, T, GREF)[None]) - 1)) < 1e-12
    assert ch.ch_m_entry(3.0, 0.7, 1.1, 0) == (3.0 * 0.7) * 1.1 and ch.ch_m_entry(3.0, 0.7, 1.1, 1) == 1.0 + (3.0 * 0.7) * 1.1
    assert ch.ch_value(10.0, 1.5) == 0.5 * 10.0 - 1.5


# ---------------------------------------------------------------- refusals ----------------------------------------------------
def test_engine_refusals_before_any_launch():
    """configured, never prepared: every refusal comes before the device is touched"""
    from pta_replicator_amd import engine_clnl
    from test_lnl_host import _engine
    eng = _engine()
    n = eng.P
    U = np.eye(n) + 0.1
    with pytest.raises(ValueError, match="5 ORFs"):
        eng.prepare_correlated_likelihood(orfs=("hd", "curn", "monopole", "dipole", U))
    with pytest.raises(ValueError, match="0 ORFs"):
        eng.prepare_correlated_likelihood(orfs=())
    with pytest.raises(ValueError, match="unknown ORF 'quadrupole'"):
        eng.prepare_correlated_likelihood(orfs=("hd", "quadrupole"))
    with pytest.raises(ValueError, match="symmetric"):
        eng.prepare_correlated_likelihood(orfs=(np.triu(U),))
    with pytest.raises(ValueError, match="positive semi-definite"):
        eng.prepare_correlated_likelihood(orfs=(np.eye(n) - 2.0 * np.ones((n, n)) / n,))
    with pytest.raises(ValueError, match="rank 0"):
        eng.prepare_correlated_likelihood(orfs=(np.zeros((n, n)),))
    with pytest.raises(ValueError, match="finite"):
        eng.prepare_correlated_likelihood(orfs=(np.eye(n + 1),))
    with pytest.raises(ValueError, match="components"):
        eng.prepare_correlated_likelihood(components=33)
    eng.P = 300                                                               # 300 * 64 projections do not fit pta_clnl_mix's LDS
    with pytest.raises(ValueError, match="hold"):
        eng.prepare_correlated_likelihood(components=32, orfs=("curn",))
    eng.P = n
    with pytest.raises(ValueError, match="timing_model"):
        eng.prepare_correlated_likelihood(timing_model="full")
    assert not eng._prepared
    G = 3
    for key in ("rn_log10_A", "rn_gamma", "gwb_log10_hc", "gwb_clm", "wn_efac", "wn_log10_equad", "chrom_log10_A", "chrom_gamma", "cw_log10_mc",
                "bwm_log10_h"):
        for call in (lambda g: eng.correlated_log_likelihood(None, g), lambda g: eng.generate_correlated_lnl(2, g)):
            with pytest.raises(ValueError, match=f"{key}.*intrinsic noise of this likelihood is the configured one"):
                call({"gwb_log10_A": np.full(G, -14.0), key: np.zeros(G)})
    with pytest.raises(ValueError, match="unknown key"):
        eng.correlated_log_likelihood(None, {"gwb_amplitude": np.zeros(G)})
    with pytest.raises(ValueError, match="dict"):
        eng.correlated_log_likelihood(None, [1, 2])
    with pytest.raises(ValueError, match="not prepared"):
        eng.correlated_log_likelihood(None, {"gwb_log10_A": np.full(G, -14.0)})
    with pytest.raises(ValueError, match="not prepared"):
        eng.generate_correlated_lnl(2, {"gwb_log10_A": np.full(G, -14.0)})
    eng._clnl = {"engine_plan": object()}
    eng._prepared, eng.plan = True, object()
    with pytest.raises(ValueError, match="re-prepared since"):
        eng.correlated_log_likelihood(None, {"gwb_log10_A": np.full(G, -14.0)})
    eng._prepared = False
    del eng.plan
    # the grid's values: an amplitude given nowhere (this engine has no GWB configured), shapes, non-finite entries
    with pytest.raises(ValueError, match="given nowhere"):
        engine_clnl.check_grid({"gwb_gamma": np.full(G, 4.0)}, None, GREF)
    with pytest.raises(ValueError, match="given nowhere"):
        engine_clnl.check_grid({}, None, GREF)
    lA, g = engine_clnl.check_grid({"gwb_gamma": np.full(G, 4.0)}, -14.3, GREF)
    assert np.array_equal(lA, np.full(G, -14.3)) and np.array_equal(g, np.full(G, 4.0))
    lA, g = engine_clnl.check_grid({}, -14.3, GREF)
    assert lA.shape == (1,) and g[0] == GREF
    for bad, msg in (({"gwb_log10_A": np.zeros((G, 2))}, "shape"), ({"gwb_log10_A": -14.0}, "shape"), ({"gwb_log10_A": np.array([-14.0, np.nan])}, "non-finite"),
                     ({"gwb_log10_A": np.zeros(G), "gwb_gamma": np.zeros(G + 1)}, "leading axis")):
        with pytest.raises(ValueError, match=msg):
            engine_clnl.check_grid(bad, None, GREF)
    grid, shape = eng.theta_grid(gwb_log10_A=[-15.0, -14.0], gwb_gamma=[3.0, 4.0, 5.0])
    assert shape == (2, 3) and engine_clnl.check_grid(grid, None, GREF)[0].shape == (6,)
    assert not eng._prepared
