"""Continuous-wave F-statistics (incoherent Fp, earth-term coherent Fe) of the ReplicaEngine's realisations, per realisation, on the
device.

``prepare_f_statistic(freqs, sky)`` builds the realisation-independent operands on the host from the noise model ``prepare()`` holds
(pta_replicator_amd/f_statistic.py: W_a = E_a^T P_a^-1 over the frequency grid, G_aj^-1, the antenna patterns phi and M_js^-1) and
uploads them once; ``f_statistic(rows)`` then costs per chunk of realisations

    pta_fstat_project   Q[r, a, :] = W_a r_a                       ragged grouped GEMM over all pulsars (fp64 MFMA), 2 J columns
    pta_fstat_fp        Fp[r, j] = 1/2 sum_a q^T G_aj^-1 q          ascending pulsars
    pta_fstat_fe        Fe[r, j, s] = 1/2 N^T M_js^-1 N             N = sum_a phi_as (x) q_raj on the matrix cores, never stored;
                                                                   the full map, or (sky_max) its maximum and argmax per (r, j)

and ``generate_f_statistic(R)`` runs generate / generate_td / generate(theta=...) chunk by chunk into one reused buffer with the
statistics behind each chunk, keeping only the statistics.  A realisation's statistics are bit-identical whatever chunk, row or
output mode they are computed in.

The noise weights are the configured ones (white noise + ECORR + red noise, optionally the GWB auto-term, timing model
marginalised): a statistic matched to per-realisation noise parameters theta is out of scope, as are the pulsar term and frequency
evolution across the data span.

The low-rank columns of the noise model, the chunk rule, the workspace with the projection and the loops over given and generated
rows are engine_stats.SkyStatisticsMixin's, shared with the BWM statistic; the argument checks, the host noise model and the rows and
state checks are its base StatisticsMixin's, shared with the optimal statistic and the likelihood too.
"""
import torch

from . import _chrom, _cproc, _cw, _lib, device as dv
from . import f_statistic as fst
from ._position import ra_dec
from .engine_stats import SkyStatisticsMixin, check_components, check_timing_model


class FStatisticMixin(SkyStatisticsMixin):
    def prepare_f_statistic(self, freqs, sky=None, timing_model="spin", gwb_auto=None, components=14, gamma=13. / 3.):
        """W, G^-1 (and with a sky grid phi, M^-1) of the array under the configured noise model (white noise + ECORR + red noise,
        optionally the GWB auto-term), uploaded once.  Returns self.

        freqs: [J] GW frequencies in Hz (finite, > 0); sky: None for Fp only, or a (cos_gwtheta [S], gwphi [S]) pair - the sky grid of
        Fe, in the angles of theta's cw_cos_gwtheta / cw_gwphi (needs at least two pulsars); timing_model: "spin", "astrometric" or
        None; gwb_auto: None = the configured GWB amplitude if a GWB is set, else no GW term in C_a; a float = that log10_A; False =
        off; components, gamma: the frequencies k / T and spectral index of that auto-term, as in prepare_optimal_statistic.

        The weights are those of the configured noise model for every realisation: a statistic matched to per-realisation theta is
        out of scope.  A frequency at which a pulsar's sin / cos pair is not constrained (one the spin-down fit absorbs) is refused."""
        f = fst.check_freqs(freqs)
        sky = fst.check_sky(sky)
        check_timing_model(timing_model)
        check_components(components, columns="")
        J = len(f)
        if 2 * J > _lib.FSTAT_CMAX:
            raise ValueError(f"{J} frequencies: one preparation holds at most {_lib.FSTAT_CMAX // 2}")
        if sky is not None and self.P < 2:
            raise ValueError("the coherent Fe statistic needs at least two pulsars; Fp alone (sky=None) works for one")
        if sky is not None and self.P > _lib.FSTAT_PMAX:
            raise ValueError(f"the Fe kernel holds at most {_lib.FSTAT_PMAX} pulsars, got {self.P}")
        self._stats_need_noise("the F-statistic")
        if 2 * J * self.n_toa * 8 > int(self.workspace_bytes):
            raise ValueError(f"the projection operator [2 J = {2 * J}, n_toa = {self.n_toa}] takes {2 * J * self.n_toa * 8} bytes, more than "
                             f"workspace_bytes = {int(self.workspace_bytes)}: use fewer frequencies per preparation or raise workspace_bytes")
        gw_lA = self._stats_gwb_auto(gwb_auto)
        toas, sigma2, epoch_of, ecorr, F_rn, phi_rn, M = self._stats_noise_model(timing_model)
        F_low, phi_low = self._sky_low_rank(toas, F_rn, phi_rn, gw_lA, components, gamma)
        phat = _cw.pulsar_vectors([ra_dec(p) for p in self.psrs]) if sky is not None else None
        plan = fst.prepare(toas, sigma2, f, phat=phat, sky=sky, epoch_of=epoch_of, ecorr=ecorr, F_rn=F_low, phi_rn=phi_low, M=M)
        self._fs = dict(plan=plan, engine_plan=self.plan, J=J, C=2 * J, S=plan.S, Wt=dv.f64(plan.Wt()), off=dv.i32(self.off), Ginv=dv.f64(plan.Ginv_packed()),
                        freqs=dv.f64(f), phi=None, Minv=None, ntile=0, ws=None)
        if sky is not None:
            self._fs.update(phi=dv.f64(plan.phi), Minv=dv.f64(plan.Minv_packed()), ntile=int(_lib.lib.pta_fstat_fe_tiles(plan.S)))
        return self

    def _fs_state(self, what, sky_max=False):
        st = self._stats_state("_fs", "the F-statistic", "prepare_f_statistic", what)
        if sky_max and st["phi"] is None:
            raise ValueError(f"{what}: sky_max=True needs a sky grid (prepare_f_statistic(freqs, sky=...))")
        return st

    def _fs_out(self, st, R, sky_max):
        J, S = st["J"], st["S"]
        out = {"fp": dv.empty((R, J)), "fe": None, "fe_max": None, "fe_arg": None}
        if st["phi"] is not None:
            if sky_max:
                out["fe_max"], out["fe_arg"] = dv.empty((R, J)), dv.empty((R, J), dtype=torch.int32)
            else:
                out["fe"] = dv.empty((R, J, S))
        return out

    def _fs_result(self, st, out):
        res = {"fp": out["fp"], "freqs": st["freqs"]}
        res.update({k: out[k] for k in ("fe", "fe_max", "fe_arg") if out[k] is not None})
        return res

    def _fs_launch(self, rows, n, lo, out):
        """rows [n, n_toa] = realisations lo .. lo+n-1 of the call -> rows lo .. of out: the projection into the reused Q buffer
        (_sky_project), pta_fstat_fp, pta_fstat_fe - all on the current stream"""
        st = self._fs
        P, J, S = self.P, st["J"], st["S"]
        sky_max = out["fe_max"] is not None
        ws = self._sky_project(st, rows, n, sky_max)
        s, Q = dv.stream_ptr(), ws["Q"]
        _lib.call("pta_fstat_fp", dv.ptr(Q), P * 2 * J, P, J, n, dv.ptr(st["Ginv"]), dv.row_ptr(out["fp"], lo), J, s)
        if st["phi"] is None:
            return
        if sky_max:
            _lib.call("pta_fstat_fe", dv.ptr(Q), P * 2 * J, P, J, n, dv.ptr(st["phi"]), S, dv.ptr(st["Minv"]), None, 0,
                      dv.row_ptr(out["fe_max"], lo), J, dv.row_ptr(out["fe_arg"], lo), J, dv.ptr(ws["pv"]), dv.ptr(ws["pa"]), s)
        else:
            _lib.call("pta_fstat_fe", dv.ptr(Q), P * 2 * J, P, J, n, dv.ptr(st["phi"]), S, dv.ptr(st["Minv"]),
                      dv.row_ptr(out["fe"], lo), J * S, None, 0, None, 0, None, None, s)

    def f_statistic(self, rows, sky_max=False):
        """Fp and Fe of every realisation of rows [R, n_toa] (a float64 device tensor with unit column stride: any output of generate,
        generate_td, generate_sampled, or the caller's own residuals).  Returns a dict of device tensors: fp [R, J], freqs [J]; with a
        sky grid fe [R, J, S], or with sky_max=True fe_max [R, J] and fe_arg [R, J] (int32: the sky index of the maximum, the lowest
        on ties) - the map is then never written.  The noise weights are the configured ones (no per-realisation theta).  Rows are
        processed in chunks that keep the workspace (Q, the per-tile maxima of sky_max) within workspace_bytes; the returned tensors
        are the caller's result and lie outside that budget: the full map takes R J S 8 bytes, and sky_max=True is the way to stay
        small."""
        st = self._fs_state("f_statistic", sky_max)
        return self._fs_result(st, self._sky_rows(st, self._fs_launch, lambda R: self._fs_out(st, R, sky_max), rows, sky_max))

    def generate_f_statistic(self, R, r0=0, theta=None, td=False, chunk=1024, sky_max=False):
        """Fp / Fe of realisations r0 .. r0+R-1, generated chunk by chunk into one reused [chunk, n_toa] buffer (generate, generate_td
        with td=True, or generate(theta=...) with theta = per-realisation parameters of the R realisations, cw_* keys included); only
        the statistics are kept.  Same results as f_statistic(generate(R, r0, ...), sky_max), bit for bit, whatever the chunk.  The
        chunk is cut so that the buffer and Q stay within workspace_bytes.  theta only shapes the data: the statistic's noise weights
        stay the configured ones."""
        if td:
            _chrom.refuse_td(self._chrom, "generate_f_statistic(td=True)")
            _cproc.refuse_td(self._cproc, "generate_f_statistic(td=True)")
        st = self._fs_state("generate_f_statistic", sky_max)
        out = self._sky_generate("generate_f_statistic", st, lambda: self._fs_state("generate_f_statistic"), self._fs_launch,
                                 lambda R: self._fs_out(st, R, sky_max), R, r0, theta, td, chunk, sky_max)
        return self._fs_result(st, out)
