"""Earth-term burst-with-memory (BWM) matched filter of the ReplicaEngine's realisations, per realisation, on the device.

``prepare_bwm_statistic(t0_mjd, sky)`` builds the realisation-independent operands on the host from the noise model ``prepare()`` holds
(pta_replicator_amd/bwm_statistic.py: W_a = e_a^T P_a^-1 over the epoch grid, g_aj, the antenna patterns phi and M_js^-1) and uploads
them once; ``bwm_statistic(rows)`` then costs per chunk of realisations

    pta_fstat_project   Q[r, a, :] = W_a r_a                       the F-statistic's ragged grouped GEMM (fp64 MFMA), J columns (+ a pad)
    pta_bwm_stat        Fb[r, j, s] = 1/2 N^T M_js^-1 N             N = sum_a phi_as q_raj on the matrix cores, never stored; the full
                                                                   map (and A = M^-1 N), or (sky_max) its maximum and argmax per (r, j)

and ``generate_bwm_statistic(R)`` runs generate / generate_td / generate(theta=...) chunk by chunk into one reused buffer with the
statistic behind each chunk, keeping only the statistic.  A realisation's values are bit-identical whatever chunk, row or output mode
they are computed in.

The noise weights are the configured ones (white noise + ECORR + red noise, optionally the GWB auto-term, timing model marginalised).
Out of scope: the pulsar term and the single-pulsar ramp statistic, a statistic matched to per-realisation theta, more than one burst
per realisation, maximising over a continuous epoch.

The low-rank columns of the noise model, the chunk rule, the workspace with the projection and the loops over given and generated
rows are engine_stats.SkyStatisticsMixin's, shared with the F-statistic; the argument checks, the host noise model and the rows and
state checks are its base StatisticsMixin's, shared with the optimal statistic and the likelihood too.
"""
import torch

from . import _chrom, _cproc, _cw, _lib, device as dv
from . import bwm_statistic as bst
from . import f_statistic as fst
from ._position import ra_dec
from .engine_stats import SkyStatisticsMixin, check_components, check_timing_model


class BwmStatisticMixin(SkyStatisticsMixin):
    def prepare_bwm_statistic(self, t0_mjd, sky, timing_model="spin", gwb_auto=None, components=14, gamma=13. / 3.):
        """W, g (and phi, M^-1 on the sky grid) of the array under the configured noise model (white noise + ECORR + red noise,
        optionally the GWB auto-term), uploaded once.  Returns self.

        t0_mjd: [J] burst epochs (MJD, finite), the grid of theta's bwm_t0_mjd; sky: a (cos_gwtheta [S], gwphi [S]) pair, the sky grid
        in the angles of theta's bwm_cos_gwtheta / bwm_gwphi (mandatory; needs at least two pulsars); timing_model: "spin",
        "astrometric" or None; gwb_auto, components, gamma: the GWB auto-term of C_a, as in prepare_f_statistic.

        A pulsar whose data do not constrain the ramp of an epoch (all its TOAs before it, or all after it so that the spin-down fit
        absorbs the ramp) contributes nothing at that epoch; an epoch fewer than two pulsars are sensitive to is refused."""
        t0 = bst.check_epochs(t0_mjd)
        if sky is None:
            raise ValueError("prepare_bwm_statistic: the sky grid is mandatory, sky = (cos_gwtheta [S], gwphi [S])")
        sky = fst.check_sky(sky)
        check_timing_model(timing_model)
        check_components(components, columns="")
        J = len(t0)
        if J > _lib.FSTAT_CMAX - 1:
            raise ValueError(f"{J} epochs: one preparation holds at most {_lib.FSTAT_CMAX - 1}")
        if self.P < 2:
            raise ValueError("the BWM statistic needs at least two pulsars")
        if self.P > _lib.FSTAT_PMAX:
            raise ValueError(f"the BWM statistic kernel holds at most {_lib.FSTAT_PMAX} pulsars, got {self.P}")
        self._stats_need_noise("the BWM statistic")
        C = J + (J & 1)
        if C * self.n_toa * 8 > int(self.workspace_bytes):
            raise ValueError(f"the projection operator [{C}, n_toa = {self.n_toa}] takes {C * self.n_toa * 8} bytes, more than "
                             f"workspace_bytes = {int(self.workspace_bytes)}: use fewer epochs per preparation or raise workspace_bytes")
        gw_lA = self._stats_gwb_auto(gwb_auto)
        toas, sigma2, epoch_of, ecorr, F_rn, phi_rn, M = self._stats_noise_model(timing_model)
        F_low, phi_low = self._sky_low_rank(toas, F_rn, phi_rn, gw_lA, components, gamma)
        phat = _cw.pulsar_vectors([ra_dec(p) for p in self.psrs])
        plan = bst.prepare(toas, sigma2, t0 * 86400.0, phat, sky, epoch_of=epoch_of, ecorr=ecorr, F_rn=F_low, phi_rn=phi_low, M=M)
        self._bs = dict(plan=plan, engine_plan=self.plan, J=J, C=plan.C, S=plan.S, Wt=dv.f64(plan.Wt()), off=dv.i32(self.off), t0_mjd=dv.f64(t0),
                        phi=dv.f64(plan.phi), Minv=dv.f64(plan.Minv_packed()), ntile=int(_lib.lib.pta_fstat_fe_tiles(plan.S)), ws=None)
        return self

    def _bs_state(self, what):
        return self._stats_state("_bs", "the BWM statistic", "prepare_bwm_statistic", what)

    @staticmethod
    def _bs_modes(what, sky_max, amplitudes):
        if sky_max and amplitudes:
            raise ValueError(f"{what}: amplitudes=True needs the full map (sky_max=True keeps the maxima only)")

    def _bs_out(self, st, R, sky_max, amplitudes):
        J, S = st["J"], st["S"]
        out = dict.fromkeys(("fb", "amp", "fb_max", "fb_arg"))
        if sky_max:
            out["fb_max"], out["fb_arg"] = dv.empty((R, J)), dv.empty((R, J), dtype=torch.int32)
        else:
            out["fb"] = dv.empty((R, J, S))
            if amplitudes:
                out["amp"] = dv.empty((R, J, S, 2))
        return out

    def _bs_result(self, st, out):
        res = {k: v for k, v in out.items() if v is not None}
        res["t0_mjd"] = st["t0_mjd"]
        return res

    def _bs_launch(self, rows, n, lo, out):
        """rows [n, n_toa] = realisations lo .. lo+n-1 of the call -> rows lo .. of out: the projection into the reused Q buffer
        (_sky_project), then pta_bwm_stat - on the current stream"""
        st = self._bs
        P, J, C, S = self.P, st["J"], st["C"], st["S"]
        sky_max = out["fb_max"] is not None
        ws = self._sky_project(st, rows, n, sky_max)
        s, Q = dv.stream_ptr(), ws["Q"]
        if sky_max:
            _lib.call("pta_bwm_stat", dv.ptr(Q), P * C, P, C, J, n, dv.ptr(st["phi"]), S, dv.ptr(st["Minv"]), None, 0, None, 0,
                      dv.row_ptr(out["fb_max"], lo), J, dv.row_ptr(out["fb_arg"], lo), J, dv.ptr(ws["pv"]), dv.ptr(ws["pa"]), s)
        else:
            _lib.call("pta_bwm_stat", dv.ptr(Q), P * C, P, C, J, n, dv.ptr(st["phi"]), S, dv.ptr(st["Minv"]), dv.row_ptr(out["fb"], lo), J * S,
                      dv.row_ptr(out["amp"], lo), 2 * J * S, None, 0, None, 0, None, None, s)

    def bwm_statistic(self, rows, sky_max=False, amplitudes=False):
        """Fb of every realisation of rows [R, n_toa] (a float64 device tensor with unit column stride: any output of generate,
        generate_td, generate_sampled, or the caller's own residuals).  Returns a dict of device tensors: fb [R, J, S] and t0_mjd [J];
        with amplitudes=True also amp [R, J, S, 2], the amplitude estimates (h cos 2psi, h sin 2psi); with sky_max=True fb_max [R, J]
        and fb_arg [R, J] (int32: the sky index of the maximum, the lowest on ties) instead - the map is then never written, and
        amplitudes is refused.  The noise weights are the configured ones (no per-realisation theta).  Rows are processed in chunks that
        keep the workspace (Q, the per-tile maxima of sky_max) within workspace_bytes; the returned tensors are the caller's result and
        lie outside that budget."""
        self._bs_modes("bwm_statistic", sky_max, amplitudes)
        st = self._bs_state("bwm_statistic")
        return self._bs_result(st, self._sky_rows(st, self._bs_launch, lambda R: self._bs_out(st, R, sky_max, amplitudes), rows, sky_max))

    def generate_bwm_statistic(self, R, r0=0, theta=None, td=False, chunk=1024, sky_max=False, amplitudes=False):
        """Fb of realisations r0 .. r0+R-1, generated chunk by chunk into one reused [chunk, n_toa] buffer (generate, generate_td with
        td=True, or generate(theta=...) with theta = per-realisation parameters of the R realisations, bwm_* and cw_* keys included);
        only the statistic is kept.  Same results as bwm_statistic(generate(R, r0, ...), sky_max, amplitudes), bit for bit, whatever
        the chunk.  The chunk is cut so that the buffer and Q stay within workspace_bytes.  theta only shapes the data: the statistic's
        noise weights stay the configured ones."""
        self._bs_modes("generate_bwm_statistic", sky_max, amplitudes)
        if td:
            _chrom.refuse_td(self._chrom, "generate_bwm_statistic(td=True)")
            _cproc.refuse_td(self._cproc, "generate_bwm_statistic(td=True)")
        st = self._bs_state("generate_bwm_statistic")
        out = self._sky_generate("generate_bwm_statistic", st, lambda: self._bs_state("generate_bwm_statistic"), self._bs_launch,
                                 lambda R: self._bs_out(st, R, sky_max, amplitudes), R, r0, theta, td, chunk, sky_max)
        return self._bs_result(st, out)
