"""Likelihood ratio of a correlated common process of the ReplicaEngine's realisations on a (log10_A, gamma) grid, on the device.

``prepare_correlated_likelihood()`` builds the theta-independent operands on the host from the noise model ``prepare()`` holds
(pta_replicator_amd/optimal_statistic.py: the OSPlan without a GWB auto-term - W_a = S^1/2 F_a^T P~_a, Z_a - and per ORF its factor
Gamma = B B^T and T = (B^T (x) I) blockdiag(Z_a) (B (x) I)) and uploads them once.  ``correlated_log_likelihood(rows, grid)`` then runs

    pta_os_project         Y[r, a, :] = W_a r_a                         every residual read once
    pta_clnl_mix           Y'[r, o, i, :] = sum_a B_o^T[i, a] Y[r, a, :]   per ORF
    pta_clnl_assemble      M_g = I + D_g T_o D_g                        per (ORF, grid chunk)
    pta_potrf_batched_ex   M_g = L_g L_g^T                              the dense Cholesky, batched over the grid chunk
    pta_clnl_rhs           V[g][:, r] = D_g Y'_r
    pta_clnl_solve         V <- L_g^-1 V, quad[g, r] = || V[:, r] ||^2   blocked forward substitution on the fp64 matrix cores
    pta_clnl_finish        lnl_ratio[g, r] = quad / 2 - sum_i ln L_g,ii

and ``generate_correlated_lnl(R, grid)`` generates chunk by chunk into the rows buffer the statistics share, with the likelihood behind
each chunk.  A (realisation, ORF, grid point) value is bit-identical whatever chunks, rows or grid points share its launches.

The model: the intrinsic noise of every pulsar (white noise, ECORR, red noise, the chromatic columns of an engine that has them) stays
at the configured values, the timing model is marginalised with a flat prior, and only the common process varies - its (log10_A,
gamma) over the grid and its ORF over the prepared ones ("hd", "monopole", "dipole", "curn" = no correlations, or a [P, P] array).  The
value is ln L(r | common process) - ln L(r | noise only); differences between ORFs are log likelihood ratios between them.  The host
front (argument checks, noise model, rows and state checks, projection, the chunked generation loop) is engine_stats.StatisticsMixin's.
"""
import ctypes

import numpy as np
import torch

from . import _chrom, _cproc, _lib, device as dv
from . import optimal_statistic as ost
from .engine_stats import StatisticsMixin, check_components, check_timing_model

GRID_KEYS = ("gwb_log10_A", "gwb_gamma")
_FIXED_PREFIXES = ("rn_", "wn_", "chrom_", "cp_", "cw_", "bwm_", "burst_", "nt_", "ce_")
_FIXED_KEYS = ("gwb_log10_hc", "gwb_clm")


def check_orfs(orfs, P):
    """the orfs argument of prepare_correlated_likelihood as a tuple of names / float64 arrays: 1 .. 4 entries, names of
    optimal_statistic.CLNL_ORF_NAMES, arrays finite, symmetric [P, P], positive semi-definite and of rank >= 1 (host only)"""
    orfs = (orfs,) if isinstance(orfs, str) or (hasattr(orfs, "ndim") and getattr(orfs, "ndim") == 2) else tuple(orfs)
    if not 1 <= len(orfs) <= _lib.CLNL_NORF:
        raise ValueError(f"{len(orfs)} ORFs: one call evaluates 1 .. {_lib.CLNL_NORF}")
    out = []
    for o in orfs:
        if isinstance(o, str):
            if o not in ost.CLNL_ORF_NAMES:
                raise ValueError(f"unknown ORF {o!r}: expected one of {ost.CLNL_ORF_NAMES} or a [P, P] array")
            out.append(o)
        else:
            m = ost._orf_array(o, P)
            ost.orf_factor(m)          # refuses a matrix that is not positive semi-definite, and rank 0
            out.append(m)
    return tuple(out)


def check_grid_keys(grid):
    """the keys of a grid dict: gwb_log10_A and gwb_gamma alone; every other key of theta is refused by name"""
    if not isinstance(grid, dict):
        raise ValueError("grid must be a dict with gwb_log10_A [G] and / or gwb_gamma [G]")
    for k in grid:
        if k in GRID_KEYS:
            continue
        if k in _FIXED_KEYS or any(str(k).startswith(p) for p in _FIXED_PREFIXES):
            raise ValueError(f"grid[{k!r}]: the intrinsic noise of this likelihood is the configured one and the common process is a power law "
                             f"with the prepared ORFs - only {list(GRID_KEYS)} vary over the grid")
        raise ValueError(f"grid[{k!r}]: unknown key (expected a subset of {list(GRID_KEYS)})")


def check_grid(grid, configured_log10_A, gamma_ref):
    """(log10_A [G], gamma [G]) float64 host arrays of a grid dict: gwb_log10_A and / or gwb_gamma [G]; a missing key takes the
    configured GWB amplitude / the prepared gamma.  Every other key of theta is refused by name: the intrinsic noise of this likelihood
    is the configured one."""
    check_grid_keys(grid)
    vals, G = {}, None
    for k, v in grid.items():
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        v = np.asarray(v, dtype=np.float64)
        if v.ndim != 1 or v.size < 1:
            raise ValueError(f"grid[{k!r}]: expected shape [G >= 1], got {v.shape}")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"grid[{k!r}]: non-finite values")
        if G is not None and len(v) != G:
            raise ValueError(f"grid[{k!r}]: leading axis {len(v)}, but the other key has shape [G = {G}]")
        G = len(v)
        vals[k] = np.ascontiguousarray(v)
    G = 1 if G is None else G
    if "gwb_log10_A" not in vals:
        if configured_log10_A is None:
            raise ValueError("grid: no gwb_log10_A and no GWB configured on the engine - the amplitude of the common process is given nowhere")
        vals["gwb_log10_A"] = np.full(G, float(configured_log10_A))
    if "gwb_gamma" not in vals:
        vals["gwb_gamma"] = np.full(G, float(gamma_ref))
    return vals["gwb_log10_A"], vals["gwb_gamma"]


class CorrelatedLikelihoodMixin(StatisticsMixin):
    def prepare_correlated_likelihood(self, components=14, gamma=13. / 3., orfs=("hd", "curn"), timing_model="spin"):
        """Operands of the likelihood ratio of a correlated common process under the configured noise model, uploaded once.

        components: n_f = 1 .. 32 frequencies k / T of the common process (T = span of the whole array); gamma: the spectral index
        where the grid gives none (and the reference index the operands are scaled with); orfs: 1 .. 4 of "hd", "monopole", "dipole",
        "curn" (no correlations) or symmetric positive semi-definite [P, P] arrays, used as given (the named ones have a unit
        diagonal); timing_model: "spin", "astrometric" or None.  Works for a single pulsar and on an engine with a chromatic process
        (its columns are part of the fixed noise)."""
        check_components(components)
        check_timing_model(timing_model)
        orfs = check_orfs(orfs, self.P)
        if self.P * 2 * int(components) > _lib.CLNL_YMAX:
            raise ValueError(f"P * 2 n_f = {self.P} * {2 * int(components)} projections per realisation exceed the {_lib.CLNL_YMAX} that pta_clnl_mix "
                             "holds in LDS: fewer components")
        self._stats_need_noise("the correlated likelihood")
        toas, sigma2, epoch_of, ecorr, F_rn, phi_rn, M = self._stats_noise_model(timing_model)
        # the OSPlan wants an ORF that does not vanish on every pair; the weights it derives from it are not used here
        osp = _os_plan(toas, sigma2, self._unit_vectors(), int(components), float(gamma), epoch_of, ecorr, F_rn, phi_rn, M)
        plan = ost.clnl_plan(osp, orfs, gamma_ref=float(gamma))
        off_yp = np.concatenate([[0], np.cumsum(plan.n)]).astype(np.int64)
        self._clnl = dict(plan=plan, engine_plan=self.plan, C=plan.C, n_orf=len(plan.names), names=list(plan.names), rho=list(plan.rho),
                          n=list(plan.n), off_yp=off_yp, T=plan.T, gamma=float(gamma), Wt=dv.f64(osp.Wt()), off=dv.i32(self.off),
                          Bt=[dv.f64(np.ascontiguousarray(B.T)) for B in plan.B], To=[dv.f64(T) for T in plan.T_orf], ws=None)
        return self

    def _clnl_state(self, what):
        return self._stats_state("_clnl", "the correlated likelihood", "prepare_correlated_likelihood", what)

    def _clnl_grid(self, st, grid):
        """(device grid, G): the validated grid as contiguous float64 device tensors {lA [G], gamma [G]}"""
        lA, gam = check_grid(grid, None if self._gw is None else self._gw.get("A"), st["gamma"])
        return {"lA": dv.f64(lA), "gamma": dv.f64(gam)}, len(lA)

    def _clnl_chunks(self, st, R, G, with_rows, chunk=None):
        """(realisations, grid points) per launch sequence: the factors of a grid chunk (every ORF: sum_o n_o^2 doubles per grid point)
        within half of workspace_bytes, then Y, Y', the right-hand sides and quad of a realisation chunk (and the generated rows) in
        what is left"""
        per_g = 8 * sum(n * n for n in st["n"])
        ws = int(self.workspace_bytes)
        g_max = max(1, min(G, (ws // 2) // per_g, 65535))     # 65535: the grid points of one launch
        n_g = -(-G // g_max)
        Gc = -(-G // n_g)
        left = max(0, ws - Gc * per_g)
        per_r = 8 * (self.P * st["C"] + int(st["off_yp"][-1]) + Gc * (max(st["n"]) + 1) + (self.n_toa if with_rows else 0))
        Rc = max(1, min(R, left // per_r))
        return (Rc if chunk is None else max(1, min(Rc, chunk))), Gc

    def _clnl_out(self, R, G, st):
        return {"ratio": dv.empty((st["n_orf"], G, R)), "R": R, "G": G, "factored": None}

    def _clnl_result(self, st, out):
        return {"lnl_ratio": out["ratio"].permute(2, 0, 1), "names": list(st["names"])}

    def _clnl_launch(self, rows, n, lo, dev, Rc, Gc, out):
        """rows [n, n_toa] = realisations lo .. lo+n-1 of the call -> columns lo .. of out, every ORF and grid chunk; on the current
        stream (the factorisation's info is read back once per factored (ORF, grid chunk))"""
        st = self._clnl
        P, C, G, R = self.P, st["C"], out["G"], out["R"]
        ntot, nmax = int(st["off_yp"][-1]), max(st["n"])
        ws = st["ws"]
        if ws is None or ws["Rc"] < Rc or ws["Gc"] < Gc:
            st["ws"] = None
            ws = st["ws"] = dict(Rc=Rc, Gc=Gc, Y=dv.empty((Rc, P * C)), Yp=dv.empty((Rc, ntot)), M=[dv.empty((Gc, m, m)) for m in st["n"]],
                                 V=dv.empty((Gc * nmax * Rc,)), quad=dv.empty((Gc * Rc,)), info=dv.zeros((Gc,), dtype=torch.int32))
            out["factored"] = None
        s = dv.stream_ptr()
        self._stats_project(st["Wt"], C, st["off"], rows, n, ws["Y"])
        for o in range(st["n_orf"]):
            _lib.call("pta_clnl_mix", dv.ptr(ws["Y"]), P * C, P, C, n, dv.ptr(st["Bt"][o]), st["rho"][o],
                      ctypes.c_void_p(ws["Yp"].data_ptr() + 8 * int(st["off_yp"][o])), ntot, s)
        gref, T = st["gamma"], st["T"]
        for g0 in range(0, G, Gc):
            ng = min(Gc, G - g0)
            lA, gam = dv.row_ptr(dev["lA"], g0), dv.row_ptr(dev["gamma"], g0)
            fresh = out["factored"] != (g0, ng)   # one grid chunk in all: its factors serve every realisation chunk of the call
            for o in range(st["n_orf"]):
                rho, m, Mo = st["rho"][o], st["n"][o], ws["M"][o]
                if fresh:
                    _lib.call("pta_clnl_assemble", dv.ptr(st["To"][o]), rho, C, gref, T, lA, gam, ng, dv.ptr(Mo), s)
                    flags = _lib.POTRF_SUBSTITUTION if m <= 2048 else 0       # the choice of red_noise.cholesky_device
                    _lib.call("pta_potrf_batched_ex", dv.ptr(Mo), m, m, m * m, ng, dv.ptr(ws["info"]), flags, s)
                    bad = ws["info"][:ng].cpu().numpy()
                    if np.any(bad != 0):
                        g = int(np.flatnonzero(bad)[0])
                        raise np.linalg.LinAlgError(f"correlated likelihood: M_g of grid point {g0 + g} (ORF {st['names'][o]!r}) is not positive "
                                                    f"definite (leading minor {int(bad[g])})")
                _lib.call("pta_clnl_rhs", ctypes.c_void_p(ws["Yp"].data_ptr() + 8 * int(st["off_yp"][o])), ntot, rho, C, n, gref, T, lA, gam, ng,
                          dv.ptr(ws["V"]), n, s)
                _lib.call("pta_clnl_solve", dv.ptr(Mo), m, ng, dv.ptr(ws["V"]), n, n, dv.ptr(ws["quad"]), n, s)
                _lib.call("pta_clnl_finish", dv.ptr(Mo), m, ng, dv.ptr(ws["quad"]), n, n,
                          ctypes.c_void_p(out["ratio"].data_ptr() + 8 * ((o * G + g0) * R + lo)), R, s)
            if fresh:
                out["factored"] = (g0, ng) if Gc >= G else None
        self._clnl_grid_keep = dev   # the launches above read these buffers asynchronously

    def correlated_log_likelihood(self, rows, grid):
        """ln L(r | common process, ORF) - ln L(r | noise only) of every realisation of rows [R, n_toa] (a float64 device tensor with unit
        column stride, as log_likelihood takes them) for every prepared ORF at every grid point.

        grid: a dict with gwb_log10_A [G] and / or gwb_gamma [G] (theta_grid builds one); a missing key takes the configured GWB
        amplitude / the prepared gamma.  Every other key of theta is refused: the intrinsic noise is the configured one.  Returns
        {"lnl_ratio": [R, n_orf, G] (a device tensor, a view with free strides), "names": the ORFs}.  G and R are cut into chunks that
        keep the factors, the right-hand sides and the projections within workspace_bytes."""
        check_grid_keys(grid)
        st = self._clnl_state("correlated_log_likelihood")
        dev, G = self._clnl_grid(st, grid)
        R = self._stats_check_rows(rows)
        out = self._clnl_out(R, G, st)
        Rc, Gc = self._clnl_chunks(st, R, G, with_rows=False)
        for lo in range(0, R, Rc):
            self._clnl_launch(rows[lo:lo + Rc], min(Rc, R - lo), lo, dev, Rc, Gc, out)
        return self._clnl_result(st, out)

    def generate_correlated_lnl(self, R, grid, r0=0, theta=None, td=False, chunk=1024):
        """The likelihood ratios on grid of realisations r0 .. r0+R-1, generated chunk by chunk into the reused rows buffer (generate,
        generate_td with td=True, or generate(theta=...)); only the ratios are kept.  Same results as
        correlated_log_likelihood(generate(R, r0, ...), grid), bit for bit, whatever the chunk.  theta affects the generation only:
        the statistic weights with the configured noise, as the fixed-noise OS does."""
        if td:
            _chrom.refuse_td(self._chrom, "generate_correlated_lnl(td=True)")
            _cproc.refuse_td(self._cproc, "generate_correlated_lnl(td=True)")
        check_grid_keys(grid)
        st = self._clnl_state("generate_correlated_lnl")
        R, r0, chunk = int(R), int(r0), int(chunk)
        if R < 1 or chunk < 1 or r0 < 0:
            raise ValueError(f"generate_correlated_lnl: R={R}, chunk={chunk} must be >= 1 and r0={r0} >= 0")
        dev, G = self._clnl_grid(st, grid)
        hyper, cw = self._theta_parts(theta, R, td=td)   # all of theta, before the first chunk is launched
        Rc, Gc = self._clnl_chunks(st, R, G, with_rows=True, chunk=chunk)
        out = self._clnl_out(R, G, st)
        for lo, n, rows in self._stats_generate_chunks(lambda: self._clnl_state("generate_correlated_lnl"), R, r0, hyper, cw, td, Rc):
            self._clnl_launch(rows, n, lo, dev, Rc, Gc, out)
        return self._clnl_result(st, out)


def _os_plan(toas, sigma2, pos, components, gamma, epoch_of, ecorr, F_rn, phi_rn, M):
    """the OSPlan without a GWB auto-term (W, Z at gamma).  A single pulsar has no pairs and OSPlan's pair weights are undefined:
    its W and Z come from pulsar_operator directly, in a plan with empty pair lists."""
    P = len(toas)
    if P >= 2:
        return ost.prepare(toas, sigma2, pos, components=components, gamma=gamma, orfs=("monopole",), epoch_of=epoch_of, ecorr=ecorr, F_rn=F_rn,
                           phi_rn=phi_rn, gw_amp2=0.0, M=M)
    nf, T, _, F = ost.array_basis(toas, components, None)
    S = ost.unit_spectrum(nf, T, gamma)
    W, Z = ost.pulsar_operator(sigma2[0], F[0], S, ost.pick(epoch_of, 0), ost.pick(ecorr, 0), ost.pick(F_rn, 0), ost.pick(phi_rn, 0), 0.0, ost.pick(M, 0))
    return _SinglePulsarPlan(W, Z, S, float(T))


class _SinglePulsarPlan:
    """what clnl_plan and project read of an OSPlan, for P = 1"""

    def __init__(self, W, Z, S, T):
        self.W, self.Z, self.S, self.T = [W], Z[None], S, T
        self.P, self.C = 1, W.shape[0]
        self.off = np.array([0, W.shape[1]], dtype=np.int64)
        self.pair_a = self.pair_b = np.zeros(0, dtype=np.int32)
        self.cos_zeta = np.zeros(0)

    def Wt(self):
        return self.W[0]
