"""The host front the per-realisation statistics of the ReplicaEngine share (engine_os.py, engine_lnl.py, engine_fstat.py, engine_bwm.py): the
argument checks of their prepare_* calls, the noise model prepare() holds pulled back to the host, the checks of rows and of a
prepared state, theta of the matched noise model on the device, the blocked pta_os_project, and the chunked generation loop with its
one rows buffer.  What differs per statistic (its operands, its chunk arithmetic, its kernels) stays in its own mixin.  The two
statistics over a sky grid (F-statistic, BWM) share more - the low-rank columns of their host plans, the chunk rule, the workspace
behind pta_fstat_project and the loops over given and generated rows: SkyStatisticsMixin below.
"""
import ctypes

import numpy as np
import torch

from . import _hyper, _lib, device as dv
from . import optimal_statistic as ost


def check_components(components, columns=" (2 n_f <= 64 columns)"):
    if isinstance(components, bool) or not isinstance(components, (int, np.integer)) or not 1 <= int(components) <= 32:
        raise ValueError(f"components={components!r}: an integer 1 .. 32{columns}")


def check_timing_model(timing_model):
    if timing_model not in ("spin", "astrometric", None):
        raise ValueError(f"timing_model={timing_model!r} must be 'spin', 'astrometric' or None")


class StatisticsMixin:
    def _stats_gwb_auto(self, gwb_auto):
        """log10 amplitude of the GWB auto-term (None = no auto-term) of a prepare_* call's gwb_auto: None = the configured GWB if one
        is set, False = off, a float = that log10_A"""
        if gwb_auto is None:
            return float(self._gw["A"]) if self._gw is not None else None
        if gwb_auto is False:
            return None
        if isinstance(gwb_auto, (bool, np.bool_)):
            raise ValueError("gwb_auto: None, a log10 amplitude, or False")
        return float(gwb_auto)

    def _stats_need_noise(self, who):
        if self._wn is None:
            raise ValueError(f"{who} needs measurement noise (set_white_noise): without it the noise covariance is singular")

    def _stats_noise_model(self, timing_model):
        """(toas, sigma2, epoch_of, ecorr, F_rn, phi_rn, M): the noise model prepare() holds, as per-pulsar host arrays in the form
        the plan builders of optimal_statistic.py / f_statistic.py take (None where the engine has no ECORR / red noise / timing
        model); prepares the engine if it is not.  F_rn / phi_rn are the low-rank part of C_a: the red-noise columns, then - on an engine
        with a chromatic process - its weighted columns w . F_chrom with phi_chrom (the matched OS and the likelihood, whose columns are
        the red noise's alone, refuse such an engine before they get here)"""
        if not self._prepared:
            self.prepare()
        from .simulate import timing_design_matrix
        P = self.P
        toas = [m * 86400.0 for m in self.mjd]
        wa, wb = self.d_wn_a.cpu().numpy(), self.d_wn_b.cpu().numpy()
        sigma2 = [wa[self.off[a]:self.off[a + 1]] ** 2 + wb[self.off[a]:self.off[a + 1]] ** 2 for a in range(P)]
        epoch_of = ecorr = F_rn = phi_rn = None
        if self._ec is not None:
            epoch_of, ecorr = self.epoch_of, self.ecorrvec
        if self.plan.rn_k:
            F_rn = [self._rn_basis_host(a) for a in range(P)]
            phi_rn = [self.rn_amp[a] ** 2 for a in range(P)]
        if self._chrom is not None:   # the chromatic columns w . F_chrom join the low-rank part beside the red-noise ones
            F_ch, phi_ch = self._chrom_low_rank_host()
            F_rn = F_ch if F_rn is None else [np.concatenate([x, y], axis=1) for x, y in zip(F_rn, F_ch)]
            phi_rn = phi_ch if phi_rn is None else [np.concatenate([x, y]) for x, y in zip(phi_rn, phi_ch)]
        if self._cproc:   # and the auto-term of every common process (add_common_process): F with sum_p Gamma_p,aa phi_p, in the same place
            F_cp, phi_cp = self._cproc_low_rank_host()
            F_rn = F_cp if F_rn is None else [np.concatenate([x, y], axis=1) for x, y in zip(F_rn, F_cp)]
            phi_rn = phi_cp if phi_rn is None else [np.concatenate([x, y]) for x, y in zip(phi_rn, phi_cp)]
        M = None if timing_model is None else [timing_design_matrix(t, model=timing_model)[0] for t in toas]
        return toas, sigma2, epoch_of, ecorr, F_rn, phi_rn, M

    def _rn_basis_host(self, a):
        """the red-noise basis [N_a, K] prepare() put on the device (pta_rn_basis: sin / cos of 2 pi f t per mode, t = TDB seconds;
        libstempo convention: cos / sin of t - t[0])."""
        t = self.tdb_s[a]
        f = self.rn_freqs[a]
        lib_conv = self._rn["libstempo"]
        arg = 2 * np.pi * ((t - t[0]) if lib_conv else t)[:, None] * f[None, :]
        F = np.empty((len(t), 2 * len(f)))
        F[:, 0::2], F[:, 1::2] = (np.cos(arg), np.sin(arg)) if lib_conv else (np.sin(arg), np.cos(arg))
        return F

    def _stats_state(self, attr, who, prepare, what):
        """the state dict prepare_*() left in self.<attr>, refused where it is missing or older than the engine's plan"""
        st = getattr(self, attr, None)
        if st is None:
            raise ValueError(f"{what}: {who} is not prepared ({prepare} first)")
        if not self._prepared or st["engine_plan"] is not self.plan:
            raise ValueError(f"{what}: the engine was re-configured or re-prepared since {prepare}(): call it again")
        return st

    def _stats_check_rows(self, rows):
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.device.type != "cuda":
            raise ValueError("rows must be a float64 device tensor")
        if rows.dim() != 2 or rows.shape[1] != self.n_toa or rows.shape[0] < 1:
            raise ValueError(f"rows must be [R >= 1, {self.n_toa}], got {tuple(rows.shape)}")
        if rows.stride(1) != 1 or rows.stride(0) < self.n_toa:
            raise ValueError(f"rows must have unit column stride and row stride >= {self.n_toa}, got strides {rows.stride()}")
        return int(rows.shape[0])

    def _stats_theta_device(self, gw, K_rn, th, R):
        """theta (or a grid with G in place of R) validated by _hyper.check_theta_os -> contiguous float64 device tensors as
        pta_os_matched_prior reads them, {rn_log10_A, rn_gamma: [R, P] or None (every pulsar as configured), gw_log10_A, gw_gamma: [R]
        or None, gw_log10_hc: [R, M] or None}.  gw: the prepared auto-term (log10_A, gamma) or None, K_rn: the red-noise columns of
        the prepared operands.  Keys not given are filled with the configured red noise / the prepared auto-term; pulsars configured
        without red noise get NaN amplitudes; gwb_log10_hc comes out in ascending node frequency."""
        dev = dict.fromkeys(("rn_log10_A", "rn_gamma", "gw_log10_A", "gw_gamma", "gw_log10_hc"))
        if _hyper.SPEC_KEY in th:
            dev["gw_log10_hc"] = self._spec_theta_device(th)
        elif gw is not None:
            for k, key, conf in (("gw_log10_A", "gwb_log10_A", gw[0]), ("gw_gamma", "gwb_gamma", gw[1])):
                dev[k] = dv.as_f64(th[key]) if key in th else torch.full((R,), conf, dtype=torch.float64, device=dv.require_gpu())
        if any(k in th for k in _hyper.RN_KEYS) and K_rn:
            self._rn_theta_device(th, R, dev)
        return dev

    def _stats_project(self, Vt, K, off, rows, n, q):
        """q[n, P K] = the K operator rows Vt [K, n_toa] against rows [n, n_toa], per pulsar: pta_os_project per block of
        _lib.OS_CMAX operator rows, block k0 at column P k0 of q, on the current stream"""
        P, s = self.P, dv.stream_ptr()
        for k0 in range(0, K, _lib.OS_CMAX):
            _lib.call("pta_os_project", dv.row_ptr(Vt, k0), self.n_toa, min(_lib.OS_CMAX, K - k0), dv.ptr(off), P, ctypes.c_void_p(rows.data_ptr()),
                      rows.stride(0), n, ctypes.c_void_p(q.data_ptr() + 8 * P * k0), P * K, s)

    def _stats_generate_chunks(self, state, R, r0, hyper, cw, td, chunk):
        """realisations r0 .. r0+R-1 generated chunk by chunk (generate_td with td, else _generate with theta's parts hyper / cw, cw =
        its deterministic keys, cw_* and bwm_*) into
        the one [>= chunk, n_toa] rows buffer every statistic shares, grown on demand: yields (lo, n, rows [n, n_toa]) per chunk.
        state() re-validates the caller's prepared state after every chunk (generation may (re)prepare the engine)."""
        buf = getattr(self, "_stats_rows", None)
        if buf is None or buf.shape[0] < chunk:
            self._stats_rows = None
            buf = self._stats_rows = dv.empty((chunk, self.n_toa))

        def rows_of(part, lo, n):
            return None if part is None else {k: v[lo:lo + n] for k, v in part.items()}
        for lo in range(0, R, chunk):
            n = min(chunk, R - lo)
            rows = buf[:n]
            if td:
                self.generate_td(n, r0=r0 + lo, out=rows)
                if cw:
                    self._det_apply(rows_of(cw, lo, n), n, rows)
            else:
                self._generate(n, r0 + lo, rows, rows_of(hyper, lo, n), rows_of(cw, lo, n))
            state()
            yield lo, n, rows


class SkyStatisticsMixin(StatisticsMixin):
    """What the sky-grid statistics share beyond that (engine_fstat.py: Fp / Fe over a frequency grid, engine_bwm.py: the burst filter over
    an epoch grid).  Both project the rows on C operator rows per pulsar with pta_fstat_project and hand Q [n, P C] to their own
    kernels.  A statistic keeps its state dict (J, C, S, ntile, Wt, off, ws, ...) in an attribute of its own and passes it in as st; its
    launch(rows [n, n_toa], n, lo, out) puts realisations lo .. lo+n-1 of the call into rows lo .. of out = make_out(R)."""

    @staticmethod
    def _sky_low_rank(toas, F_rn, phi_rn, gw_lA, components, gamma):
        """(F_rn, phi_rn) of a host plan: per pulsar the low-rank part of C_a, the red-noise columns of _stats_noise_model (or None), then
        the GWB auto-term of log10 amplitude gw_lA (or None) on the frequencies k / T, k <= components; (None, None) without either"""
        P = len(toas)
        F_low, phi_low = [[] for _ in range(P)], [[] for _ in range(P)]
        if F_rn is not None:
            for a in range(P):
                F_low[a].append(F_rn[a])
                phi_low[a].append(phi_rn[a])
        if gw_lA is not None:
            T = max(float(np.max(t)) for t in toas) - min(float(np.min(t)) for t in toas)
            S = ost.unit_spectrum(int(components), T, float(gamma))
            for a in range(P):
                F_low[a].append(ost.fourier_basis(toas[a], int(components), T))
                phi_low[a].append(10.0 ** (2 * gw_lA) * S)
        if not F_low[0]:
            return None, None
        return [np.concatenate(x, axis=1) for x in F_low], [np.concatenate(x) for x in phi_low]

    def _sky_chunk(self, st, R, sky_max, with_rows):
        """realisations per launch sequence: Q [P, C], the per-tile maxima of sky_max (and the generated rows) within workspace_bytes.
        The outputs of all R realisations are the call's result, not workspace."""
        per_real = 8 * self.P * st["C"] + (12 * st["J"] * st["ntile"] if sky_max else 0) + (8 * self.n_toa if with_rows else 0)
        return max(1, min(R, int(self.workspace_bytes) // per_real))

    def _sky_project(self, st, rows, n, sky_max):
        """Q [n, P C] of rows [n, n_toa] by pta_fstat_project on the current stream, in the statistic's workspace st["ws"] = {n, Q, pv,
        pa} (pv / pa: the per-tile maxima and their sky indices, with sky_max), grown on demand.  Returns the workspace."""
        P, J, C = self.P, st["J"], st["C"]
        ws = st["ws"]
        if ws is None or ws["n"] < n or (sky_max and ws["pv"] is None):
            st["ws"] = None
            ws = st["ws"] = dict(n=n, Q=dv.empty((n, P * C)), pv=dv.empty((n * J * st["ntile"],)) if sky_max else None,
                                 pa=dv.empty((n * J * st["ntile"],), dtype=torch.int32) if sky_max else None)
        _lib.call("pta_fstat_project", dv.ptr(st["Wt"]), self.n_toa, C, dv.ptr(st["off"]), P, ctypes.c_void_p(rows.data_ptr()), rows.stride(0), n,
                  dv.ptr(ws["Q"]), P * C, dv.stream_ptr())
        return ws

    def _sky_rows(self, st, launch, make_out, rows, sky_max):
        """the statistic of the given rows [R, n_toa], in chunks that keep the workspace within workspace_bytes: returns out"""
        R = self._stats_check_rows(rows)
        out = make_out(R)
        step = self._sky_chunk(st, R, sky_max, with_rows=False)
        for lo in range(0, R, step):
            launch(rows[lo:lo + step], min(step, R - lo), lo, out)
        return out

    def _sky_generate(self, what, st, state, launch, make_out, R, r0, theta, td, chunk, sky_max):
        """the statistic of realisations r0 .. r0+R-1, generated chunk by chunk (_stats_generate_chunks; state() re-validates the
        prepared state behind each chunk), the chunk cut so that the rows buffer and the workspace stay within workspace_bytes:
        returns out"""
        R, r0, chunk = int(R), int(r0), int(chunk)
        if R < 1 or chunk < 1 or r0 < 0:
            raise ValueError(f"{what}: R={R}, chunk={chunk} must be >= 1 and r0={r0} >= 0")
        hyper, det = self._theta_parts(theta, R, td=td)   # all of theta, before the first chunk is launched
        chunk = max(1, min(chunk, self._sky_chunk(st, R, sky_max, with_rows=True)))
        out = make_out(R)
        for lo, n, rows in self._stats_generate_chunks(state, R, r0, hyper, det, td, chunk):
            launch(rows, n, lo, out)
        return out
