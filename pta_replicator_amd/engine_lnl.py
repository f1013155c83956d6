"""Timing-model-marginalised Gaussian log-likelihood of the ReplicaEngine's realisations on a grid of noise parameters, on the device.

``prepare_likelihood()`` builds the theta-independent operands on the host from the noise model ``prepare()`` holds
(pta_replicator_amd/optimal_statistic.py: V = U^T P0', A = U^T P0' U, the timing-model rows G, the white-noise / ECORR weights and the
constants c_a per pulsar, U = [F_rn | F]) and uploads them once.  ``log_likelihood(rows, grid)`` then runs

    pta_os_project         q[r, a, :] = [V_a; G_a] r_a         once per block of <= 64 operator rows
    pta_lnl_quad           r0[r, a] = r_a^T P0' r_a            one streaming pass over the residuals (the timing-model fit's residual)
    pta_os_matched_prior   b[g, a, :]                          prior variances of the grid points over the mean white-noise variance
    pta_lnl_factor         L[g, a], ln det                     one factorisation per (grid point, pulsar), shared by every realisation
    pta_lnl_apply          ln L[g, a, r]                       || L^-1 D q ||^2: blocked substitution on the fp64 matrix cores, epilogue fused
    pta_lnl_reduce         ln L[g, r] = sum_a ln L[g, a, r]    ascending pulsars

and ``generate_lnl(R, grid)`` generates chunk by chunk into one reused buffer with the likelihood behind each chunk, keeping only
ln L.  A (realisation, grid point) value is bit-identical whatever chunks, rows or grid points share its launches.

The model is the matched optimal statistic's: white noise, ECORR and the timing model are fixed, the timing model is marginalised
with a flat prior, red noise sits on the red-noise columns and a common uncorrelated process with the GWB spectrum on the 2 n_f
columns of the array-wide Fourier basis.  The grid goes to the device as the matched statistic's theta does, and the rest of the host
front (argument checks, host noise model, rows and state checks, blocked projection, the chunked generation loop with its rows
buffer) is shared too: engine_stats.StatisticsMixin.
"""
import ctypes

from . import _chrom, _cproc, _cw, _hyper, _lib, device as dv
from . import optimal_statistic as ost
from .engine_stats import StatisticsMixin, check_components, check_timing_model


class LikelihoodMixin(StatisticsMixin):
    def prepare_likelihood(self, components=14, gamma=13. / 3., timing_model="spin", gwb_auto=None):
        """Operands of ln L(r | theta) under the configured noise model, uploaded once.  Works for a single pulsar; needs no ORFs.

        components: n_f = 1 .. 32 frequencies k / T of the common process (T = span of the whole array); gamma: its spectral index
        where the grid gives none; timing_model: "spin", "astrometric" or None; gwb_auto: None = the configured GWB amplitude if a
        GWB is set, else no common process; a float = that log10_A; False = off (gwb_* grid keys are then refused).
        K = red-noise columns + 2 n_f <= 128."""
        check_components(components)
        check_timing_model(timing_model)
        _chrom.refuse_matched(self._chrom, "prepare_likelihood")
        _cproc.refuse_matched(self._cproc, "prepare_likelihood")
        self._stats_need_noise("the likelihood")
        gw_lA = self._stats_gwb_auto(gwb_auto)
        K_rn = 2 * self._rn["components"] if self._rn is not None else 0
        if K_rn + 2 * int(components) > _lib.LNL_KMAX:
            raise ValueError(f"K = {K_rn} red-noise columns + {2 * int(components)} common-process columns exceeds the kernel limit of "
                             f"{_lib.LNL_KMAX}")
        toas, sigma2, epoch_of, ecorr, F_rn, _, M = self._stats_noise_model(timing_model)
        if M is not None and max(x.shape[1] for x in M) > _lib.LNL_MMAX:
            raise ValueError(f"the timing model has more than {_lib.LNL_MMAX} columns")
        plan = ost.prepare_lnl(toas, sigma2, components=int(components), epoch_of=epoch_of, ecorr=ecorr, F_rn=F_rn, M=M)
        psr_ep, ep_ptr, ep_idx, ep_g = plan.epochs()
        has_ep = len(ep_g) > 0
        self._lnl = dict(plan=plan, engine_plan=self.plan, K=plan.K, K_rn=plan.K_rn, C=plan.C, m=plan.m, Kt=plan.K + plan.m, T=plan.T,
                         Vt=dv.f64(plan.Vt()), Ht=dv.f64(plan.Ht_all()) if plan.m else None, A=dv.f64(plan.A), s=dv.f64(plan.s), c=dv.f64(plan.c), dinv=dv.f64(plan.dinv), off=dv.i32(self.off),
                         psr_ep=dv.i32(psr_ep) if has_ep else None, ep_ptr=dv.i32(ep_ptr) if has_ep else None,
                         ep_idx=dv.i32(ep_idx) if has_ep else None, ep_g=dv.f64(ep_g) if has_ep else None,
                         gw=None if gw_lA is None else (gw_lA, float(gamma)), rn_phi=dv.f64(self.rn_amp ** 2) if plan.K_rn else None, ws=None)
        return self

    def theta_grid(self, **axes):
        """(grid, shape): the flattened outer product of 1-D axes named by theta's keys (optimal_statistic.theta_grid with this
        array's P): gwb_* entries [G], rn_* entries [G, P] with the same value for every pulsar; the first axis varies slowest."""
        return ost.theta_grid(P=self.P, **axes)

    def _lnl_state(self, what):
        return self._stats_state("_lnl", "the likelihood", "prepare_likelihood", what)

    def _lnl_check_grid(self, st, grid):
        """(theta, G): the grid validated as G noise models (_hyper.check_theta_os with G in place of R), host only.  cw_* keys are
        refused: a deterministic source is not part of the likelihood's model."""
        if not isinstance(grid, dict):
            raise ValueError("grid must be a dict of theta's keys with a leading grid axis")
        rest, cw = _cw.split(grid)
        if cw:
            raise ValueError(f"grid: cw_* keys {sorted(cw)} are not part of the likelihood's noise model")
        G = None
        for k, v in rest.items():
            n = int(v.shape[0]) if hasattr(v, "shape") and len(v.shape) else (len(v) if hasattr(v, "__len__") else None)
            if n is None or n < 1:
                raise ValueError(f"grid[{k!r}]: expected a non-empty leading grid axis (shape [G] or [G, P])")
            if G is not None and n != G:
                raise ValueError(f"grid[{k!r}]: leading axis {n}, but the other keys have shape [G = {G}, ...]")
            G = n
        G = 1 if G is None else G
        return _hyper.check_theta_os(rest, G, self.P, self._rn, st["gw"] is not None), G

    def _lnl_grid_device(self, st, th, G):
        """contiguous float64 device tensors of the grid as pta_os_matched_prior reads them (the matched OS's rules: keys not given are
        filled with the configured red noise / the prepared common process, pulsars without red noise get NaN amplitudes)"""
        return self._stats_theta_device(st["gw"], st["K_rn"], th, G)

    def _lnl_chunks(self, st, R, G, per_pulsar, with_rows, chunk=None):
        """(realisations, grid points) per launch sequence: b, the operators (P K^2 8 bytes per grid point) and ln det of a grid chunk,
        q, r0 (and the generated rows) of a realisation chunk and the per-pulsar buffer within workspace_bytes"""
        P, K = self.P, st["K"]
        per_g = 8 * P * (K * K + K + 1)
        per_r = 8 * (P * (st["Kt"] + 1) + (self.n_toa if with_rows else 0))
        ws = int(self.workspace_bytes)
        g_max = max(1, min(G, (ws // 2) // per_g))
        n_g = -(-G // g_max)
        Gc = -(-G // n_g)
        left = max(0, ws - Gc * per_g)
        Rc = max(1, min(R, left // (per_r + (0 if per_pulsar else 8 * P * Gc))))
        return (Rc if chunk is None else max(1, min(Rc, chunk))), Gc

    def _lnl_out(self, R, G, per_pulsar):
        return {"lnl": dv.empty((G, R)), "lp": dv.empty((G, self.P, R)) if per_pulsar else None, "R": R, "G": G, "factored": None}

    def _lnl_result(self, out):
        res = {"lnl": out["lnl"].t()}
        if out["lp"] is not None:
            res["lnl_pulsar"] = out["lp"].permute(2, 1, 0)
        return res

    def _lnl_launch(self, rows, n, lo, dev, Rc, Gc, out):
        """rows [n, n_toa] = realisations lo .. lo+n-1 of the call -> columns lo .. of out, every grid chunk; all on the current stream"""
        st = self._lnl
        P, K, Kt, C, m, K_rn = self.P, st["K"], st["Kt"], st["C"], st["m"], st["K_rn"]
        G, R = out["G"], out["R"]
        ws = st["ws"]
        need_lp = out["lp"] is None
        if ws is None or ws["Rc"] < Rc or ws["Gc"] < Gc or (need_lp and (ws["lp"] is None or ws["lp"].numel() < Gc * P * Rc)):
            st["ws"] = None
            ws = st["ws"] = dict(Rc=Rc, Gc=Gc, q=dv.empty((Rc, P * Kt)), r0=dv.empty((Rc, P)), b=dv.empty((Gc, P * K)), Lt=dv.empty((Gc, P * K * K)),
                                 logdet=dv.empty((Gc, P)), lp=dv.empty((Gc * P * Rc,)) if need_lp else None)
            out["factored"] = None
        s, blk = dv.stream_ptr(), _lib.OS_CMAX
        self._stats_project(st["Vt"], Kt, st["off"], rows, n, ws["q"])
        _lib.call("pta_lnl_quad", ctypes.c_void_p(rows.data_ptr()), rows.stride(0), n, dv.ptr(st["off"]), P, dv.ptr(st["dinv"]), dv.ptr(st["psr_ep"]),
                  dv.ptr(st["ep_ptr"]), dv.ptr(st["ep_idx"]), dv.ptr(st["ep_g"]), dv.ptr(ws["q"]), P * Kt, blk, K, m, dv.ptr(st["Ht"]), self.n_toa, dv.ptr(ws["r0"]), s)
        hy = self._hyper_tables() if K_rn else {}
        at = dv.row_ptr
        for g0 in range(0, G, Gc):
            ng = min(Gc, G - g0)
            if out["factored"] != (g0, ng):         # one grid chunk in all: its factors serve every realisation chunk of the call
                _lib.call("pta_os_matched_prior", ng, P, K_rn, C, dv.ptr(hy["rn_f"]) if K_rn else None, dv.ptr(hy["rn_tspan"]) if K_rn else None,
                          dv.ptr(st["rn_phi"]) if K_rn else None, at(dev["rn_log10_A"], g0), at(dev["rn_gamma"], g0), st["T"],
                          at(dev["gw_log10_A"], g0), at(dev["gw_gamma"], g0), dv.ptr(st["s"]), dv.ptr(ws["b"]), s)
                _lib.call("pta_lnl_factor", dv.ptr(st["A"]), P, K, C, ng, dv.ptr(ws["b"]), dv.ptr(ws["Lt"]), dv.ptr(ws["logdet"]), s)
                out["factored"] = (g0, ng) if Gc >= G else None
            if out["lp"] is None:
                lp, ld_g, ld_a = ctypes.c_void_p(ws["lp"].data_ptr()), P * n, n
            else:
                lp, ld_g, ld_a = ctypes.c_void_p(out["lp"].data_ptr() + 8 * (g0 * P * R + lo)), P * R, R
            _lib.call("pta_lnl_apply", dv.ptr(ws["Lt"]), dv.ptr(ws["logdet"]), dv.ptr(ws["b"]), P, K, C, ng, dv.ptr(ws["q"]), P * Kt, blk, Kt, n, dv.ptr(ws["r0"]),
                      dv.ptr(st["s"]), dv.ptr(st["c"]), lp, ld_g, ld_a, s)
            _lib.call("pta_lnl_reduce", lp, ld_g, ld_a, P, ng, n, ctypes.c_void_p(out["lnl"].data_ptr() + 8 * (g0 * R + lo)), R, s)
        self._lnl_grid_keep = dev   # the launches above read these buffers asynchronously

    def log_likelihood(self, rows, grid, per_pulsar=False):
        """ln L of every realisation of rows [R, n_toa] (a float64 device tensor with unit column stride: any output of generate,
        generate_td, generate_sampled, or the caller's own residuals) under every noise model of grid.

        grid: a dict with the keys of theta and a leading grid axis G in place of R: gwb_log10_A [G], gwb_gamma [G], rn_log10_A [G, P],
        rn_gamma [G, P] (theta_grid builds one from 1-D axes).  Keys not given and NaN red-noise amplitudes take the configured red
        noise / the prepared common process; cw_* keys are refused.  Returns {"lnl": [R, G]} and, with per_pulsar=True, also
        {"lnl_pulsar": [R, P, G]} (device tensors, views with free strides); lnl is the sum of lnl_pulsar over the pulsars in
        ascending order.  G and R are cut into chunks that keep the workspace within workspace_bytes."""
        _chrom.refuse_noise_model(grid)
        _cproc.refuse_noise_model(grid)
        st = self._lnl_state("log_likelihood")
        R = self._stats_check_rows(rows)
        th, G = self._lnl_check_grid(st, grid)
        dev = self._lnl_grid_device(st, th, G)
        out = self._lnl_out(R, G, per_pulsar)
        Rc, Gc = self._lnl_chunks(st, R, G, per_pulsar, with_rows=False)
        for lo in range(0, R, Rc):
            self._lnl_launch(rows[lo:lo + Rc], min(Rc, R - lo), lo, dev, Rc, Gc, out)
        return self._lnl_result(out)

    def generate_lnl(self, R, grid, r0=0, theta=None, td=False, chunk=1024, per_pulsar=False):
        """ln L on grid of realisations r0 .. r0+R-1, generated chunk by chunk into one reused [chunk, n_toa] buffer (generate,
        generate_td with td=True, or generate(theta=...) with theta = per-realisation parameters of the R realisations); only ln L is
        kept.  Same results as log_likelihood(generate(R, r0, ...), grid), bit for bit, whatever the chunk.  The chunk is cut so that
        the buffer and the likelihood's workspace stay within workspace_bytes."""
        if td:
            _chrom.refuse_td(self._chrom, "generate_lnl(td=True)")
            _cproc.refuse_td(self._cproc, "generate_lnl(td=True)")
        _chrom.refuse_noise_model(grid)
        _cproc.refuse_noise_model(grid)
        st = self._lnl_state("generate_lnl")
        R, r0, chunk = int(R), int(r0), int(chunk)
        if R < 1 or chunk < 1 or r0 < 0:
            raise ValueError(f"generate_lnl: R={R}, chunk={chunk} must be >= 1 and r0={r0} >= 0")
        th, G = self._lnl_check_grid(st, grid)
        hyper, cw = self._theta_parts(theta, R, td=td)   # all of theta, before the first chunk is launched
        dev = self._lnl_grid_device(st, th, G)
        Rc, Gc = self._lnl_chunks(st, R, G, per_pulsar, with_rows=True, chunk=chunk)
        out = self._lnl_out(R, G, per_pulsar)
        for lo, n, rows in self._stats_generate_chunks(lambda: self._lnl_state("generate_lnl"), R, r0, hyper, cw, td, Rc):
            self._lnl_launch(rows, n, lo, dev, Rc, Gc, out)
        return self._lnl_result(out)
