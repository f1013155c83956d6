"""The per-realisation terms of the ReplicaEngine: theta split into its parts, the terms added after the fused launch (one CW source
or a catalogue, a burst with memory, a burst of sine-Gaussian wavelets, noise transients, chromatic events, white noise per group), theta drawn on chip from uniform boxes (set_*_prior, sample_theta) and theta
made on chip from a binned binary population (set_population, population_theta: Poisson counts, loudest-k, residual spectrum).
What the terms share is written once: the params -> add batch loop (_term_batches), the reused device tables grown on demand
(_scratch), the buffers queued launches still read (self._keep, one entry per term) and the box draw (_uniform_table).  The fixed model,
prepare(), the workspace and the generate* calls stay in engine.py.
"""
import ctypes

import numpy as np
import torch

from . import _burst, _bwm, _chrom, _chrom_event, _cproc, _cw, _hyper, _lib, _pop, _wn_hyper, device as dv
from ._position import ra_dec


class PerRealisationTermsMixin:
    # ---------------------------------------------------------------- configuration -------------
    def set_cw(self, psrTerm=True, evolve=True, phase_approx=False, tref=0.0, pdist=1.0):
        """one continuous-wave source PER REALISATION, its parameters given by the cw_* keys of theta (generate, generate_per_signal,
        generate_td, generate_os) or drawn from set_cw_prior() (generate_sampled).  The flags have add_cgw's meaning
        (deterministic.py:13-48); tref [s]; pdist [kpc], a scalar or one value per pulsar (theta's cw_pdist [R, P] overrides it).
        Adds nothing by itself; fixed sources of add_cgw / add_delays stay as they are, on top of it.  No prepare() needed."""
        self._cw = _cw.make_config(self.P, psrTerm, evolve, phase_approx, tref, pdist)
        self._cwt = None   # device tables of the previous configuration (_cw_tables)
        return self

    def set_bwm(self):
        """one burst with memory PER REALISATION (the reference's add_gw_memory, deterministic.py:822-884, Earth term), its parameters
        given by the bwm_* keys of theta (generate, generate_per_signal, generate_td, the generate_* statistics) or drawn from
        set_bwm_prior() (generate_sampled): bwm_log10_h, bwm_cos_gwtheta, bwm_gwphi, bwm_psi (the reference's bwm_pol), bwm_t0_mjd, each
        [R].  Adds nothing by itself; a fixed ramp of add_delays stays as it is, on top of it; a realisation may carry a CW source
        (set_cw) and a burst together, but one burst only.  No prepare() needed."""
        self._bwm = True
        return self

    def set_bwm_prior(self, log10_h=None, t0_mjd=None, cos_gwtheta=None, gwphi=None, psi=None):
        """uniform boxes (lo, hi) of the per-realisation burst of generate_sampled() (set_bwm configures it).  Required: log10_h and
        t0_mjd.  Defaults: cos_gwtheta (-1, 1), gwphi (0, 2 pi), psi (0, pi) (isotropic sky and polarisation).  Drawn from stream (9, 0),
        pair = label column (_bwm.COLUMNS), independently of set_hyper_prior's and set_cw_prior's parameters."""
        self._bwm_prior = _bwm.make_prior(log10_h=log10_h, t0_mjd=t0_mjd, cos_gwtheta=cos_gwtheta, gwphi=gwphi, psi=psi)
        return self

    def set_burst(self, n_wavelets=1, remove_quad=False):
        """one GW burst PER REALISATION made of n_wavelets = W <= 128 sine-Gaussian wavelets from one sky position (the reference's
        add_burst, deterministic.py:718-793, with the callables h+ = sum_w A+_w g_w cos(2 pi f_w (t - t0_w) + phi+_w), hx likewise; g =
        exp(-1/2 ((t - t0) / tau)^2), t = mjd * 86400), its parameters given by the burst_* keys of theta (pta_replicator_amd._burst:
        burst_cos_gwtheta, burst_gwphi, burst_psi [R]; burst_t0_mjd, burst_log10_tau [s], burst_log10_f [Hz], burst_log10_a_plus [s],
        burst_phase_plus, burst_log10_a_cross [s], burst_phase_cross [R, W]; optional burst_count [R], 0 = no burst) wherever the
        bwm_* keys are accepted, or drawn from set_burst_prior() (generate_sampled).  remove_quad: subtract the unweighted quadratic
        fit over every pulsar's TOAs, as the reference does (a pulsar of <= 3 TOAs gets a zero term).  Added after the BWM term by
        pta_engine_burst_add.  Adds nothing by itself; no prepare() needed."""
        self._burst = _burst.make_config(n_wavelets, remove_quad)
        return self

    def set_transients(self, n=1):
        """n = V <= 128 noise transients PER REALISATION, each a sine-Gaussian wavelet in one pulsar (the reference's
        add_noise_transient, deterministic.py:796-819), given by theta's nt_psr (integer 0 .. P-1), nt_t0_mjd, nt_log10_tau, nt_log10_f,
        nt_log10_a [s], nt_phase [R, V] and the optional nt_count [R], or drawn from set_transient_prior().  Added after the burst term
        by pta_engine_transient_add.  Adds nothing by itself; no prepare() needed."""
        self._nt = _burst.make_nt_config(n)
        return self

    def set_burst_prior(self, t0_mjd=None, log10_tau=None, log10_f=None, log10_a_plus=None, log10_a_cross=None, cos_gwtheta=None, gwphi=None,
                        psi=None, phase_plus=None, phase_cross=None):
        """uniform boxes (lo, hi) of the per-realisation wavelet burst of generate_sampled() (set_burst configures it).  Required:
        t0_mjd, log10_tau, log10_f and the two amplitudes.  Defaults: cos_gwtheta (-1, 1), gwphi (0, 2 pi), psi (0, pi), the phases
        (0, 2 pi).  The sky labels come from stream (13, 0), wavelet w from stream (13, 1 + w), pair = label column
        (_burst.SKY_COLUMNS / WAV_COLUMNS): no other label or residual moves.  Every wavelet is drawn from the same boxes."""
        self._burst_prior = _burst.make_prior(t0_mjd=t0_mjd, log10_tau=log10_tau, log10_f=log10_f, log10_a_plus=log10_a_plus,
                                              log10_a_cross=log10_a_cross, cos_gwtheta=cos_gwtheta, gwphi=gwphi, psi=psi,
                                              phase_plus=phase_plus, phase_cross=phase_cross)
        return self

    def set_transient_prior(self, t0_mjd=None, log10_tau=None, log10_f=None, log10_a=None, phase=None):
        """uniform boxes (lo, hi) of the per-realisation noise transients of generate_sampled() (set_transients configures them).
        Required: t0_mjd, log10_tau, log10_f, log10_a; phase defaults to (0, 2 pi).  Transient v comes from stream (14, v), pair = label
        column (_burst.NT_COLUMNS); nt_psr is the floor of a U(0, P) draw."""
        self._nt_prior = _burst.make_nt_prior(t0_mjd=t0_mjd, log10_tau=log10_tau, log10_f=log10_f, log10_a=log10_a, phase=phase)
        return self

    def set_chromatic_events(self, n=1, ref_freq_mhz=1400.0):
        """n = E <= 128 chromatic events PER REALISATION: deterministic terms in one pulsar that scale with the TOA's radio frequency,
        dt_i = s A (nu_ref / nu_i)^chi shape(t_i) with shape an exponential decay after t0 (kind 0, a DM dip), a cusp (1), a Gaussian bump
        (2) or the yearly sinusoid (3) (pta_replicator_amd._chrom_event, csrc/pta_chrom_event.h), given by theta's ce_psr (integer
        0 .. P-1), ce_kind (0 .. 3 or "decay" / "cusp" / "bump" / "annual"), ce_t0_mjd, ce_log10_tau [s], ce_log10_a [s at ref_freq_mhz]
        [R, E], the optional ce_log10_tau_pre (NaN = symmetric), ce_sign (-1), ce_index (2), ce_phase (0) [R, E] and ce_count [R],
        wherever the nt_* keys are accepted, or drawn from set_chromatic_event_prior().  The radio frequencies come from the pulsars
        (toas.freqs_mhz, else toas.get_freqs()); a pulsar without them, or with a non-finite or non-positive one, is refused by name.
        Added after the noise transients by pta_engine_chrom_event_add.  Adds nothing by itself; no prepare() needed.  A prior set for
        another n is dropped."""
        conf = _chrom_event.make_config(n, ref_freq_mhz)
        for p in self.psrs:
            _chrom_event.log_freq_ratio(_chrom.toa_freqs(p), conf["ref_freq_mhz"], name=f"pulsar {getattr(p, 'name', '?')}")
        self._ce, self._ce_lnu = conf, None
        if getattr(self, "_ce_prior", None) is not None and len(self._ce_prior["kind"]) != conf["E"]:
            self._ce_prior = None
        return self

    def set_chromatic_event_prior(self, kind, log10_a, psr=None, t0_mjd=None, log10_tau=None, log10_tau_pre=None, sign=-1, index=2.0,
                                  phase=(0.0, 2 * np.pi)):
        """the boxes of the per-realisation chromatic events of generate_sampled() (set_chromatic_events configures them).  Every
        argument is a scalar (the column is fixed), a box (lo, hi) (a tuple), or a list of E of those, one per slot.  kind is fixed per
        slot and never drawn; psr=None draws the pulsar as the floor of U(0, P); sign="random" is the box (-1, 1); t0_mjd and log10_tau
        are required for slots of kinds 0 - 2; log10_tau_pre=None is the NaN label (a symmetric cusp).  Slot e comes from stream (15, e),
        pair = label column (_chrom_event.COLUMNS): a label row is a function of (seed, realisation, slot) alone, and no other label or
        residual moves."""
        if getattr(self, "_ce", None) is None:
            raise ValueError("set_chromatic_event_prior: no per-realisation chromatic events configured (set_chromatic_events)")
        self._ce_prior = _chrom_event.make_prior(self._ce["E"], self.P, kind, log10_a, psr=psr, t0_mjd=t0_mjd, log10_tau=log10_tau,
                                                 log10_tau_pre=log10_tau_pre, sign=sign, index=index, phase=phase)
        return self

    def set_cw_prior(self, log10_mc=None, log10_fgw=None, log10_h=None, log10_dist=None, cos_gwtheta=None, gwphi=None, phase0=None,
                     psi=None, cos_inc=None, pdist=None, n_sources=None):
        """uniform boxes (lo, hi) of the per-realisation CW source of generate_sampled() (set_cw configures it).  Required: log10_mc
        [Msun], log10_fgw [Hz] and exactly one of log10_h / log10_dist [Mpc].  Defaults: cos_gwtheta (-1, 1), gwphi (0, 2 pi), phase0
        (0, 2 pi), psi (0, pi), cos_inc (-1, 1) (isotropic sky and orientation).  pdist [kpc]: (lo, hi) or [P, 2]; left out = set_cw's
        pdist.  Drawn from stream (8, 0), pair = label column (_cw.COLUMNS), independently of set_hyper_prior's parameters.
        n_sources = S: a catalogue of S sources per realisation, S independent draws from the same boxes, source s from stream (8, s)
        (source 0 is the single-source draw); the labels are then [R, S].  pdist stays [R, P] on stream (8, 0).  None: one source,
        labels [R]."""
        self._cw_prior = _cw.make_prior(self.P, n_sources=n_sources, log10_mc=log10_mc, log10_fgw=log10_fgw, log10_h=log10_h, log10_dist=log10_dist,
                                        cos_gwtheta=cos_gwtheta, gwphi=gwphi, phase0=phase0, psi=psi, cos_inc=cos_inc, pdist=pdist)
        return self

    def set_hyper_prior(self, gwb_log10_A=None, gwb_gamma=None, rn_log10_A=None, rn_gamma=None, gwb_log10_hc=None, gwb_clm=None,
                        wn_efac=None, wn_log10_equad=None, wn_log10_ecorr=None, chrom_log10_A=None, chrom_gamma=None, cp_log10_A=None,
                        cp_gamma=None):
        """uniform boxes of generate_sampled(): GWB keys (lo, hi); red-noise keys (lo, hi) for every pulsar or a [P, 2] array;
        gwb_log10_hc (needs set_gwb(userSpec=U [M, 2])): (lo, hi) for every node or [M, 2], box j for row j of U as given - a free
        spectrum per realisation.  gwb_clm (needs set_gwb(lmax=L >= 1)): (lo, hi) for every c_lm with l >= 1 or [(L+1)^2 - 1, 2], box j for
        column j + 1 of gwb_clm - a sky per realisation; c_00 stays as configured.  The ORF 2 sum_k c_k basis[k] is positive
        semidefinite when the power sum_lm c_lm Y_lm is positive over the sky, which every box with
        sum_{l>=1} |c_lm| max|Y_lm| <= c_00 Y_00 guarantees (real harmonics: Y_00 = 1 / sqrt(4 pi), max|Y_1m| = sqrt(3 / 4 pi)); a
        wider box may draw skies that are not, which come back flagged (generate_sampled).  wn_efac, wn_log10_equad (need
        set_white_noise) and wn_log10_ecorr (needs set_jitter): (lo, hi) for every group or [G, 2], G = len(wn_groups) or
        len(ecorr_groups), box j for group j.  chrom_log10_A, chrom_gamma (need set_chromatic_noise): (lo, hi) for every pulsar or [P, 2],
        drawn from stream (7, 6) and (7, 7), pair = pulsar (_chrom.FIELD).  cp_log10_A, cp_gamma (need add_common_process): (lo, hi) for
        every common process or [n_proc, 2], drawn from stream (7, 8) and (7, 9), pair = process (_cproc.FIELD).  Parameters left out keep their configured values.  No prepare()
        needed after a change."""
        wn_prior = _wn_hyper.make_prior(len(self.wn_groups), len(self.ecorr_groups), wn_efac=wn_efac, wn_log10_equad=wn_log10_equad,
                                        wn_log10_ecorr=wn_log10_ecorr) or None
        chrom_prior = _chrom.make_prior(self.P, chrom_log10_A=chrom_log10_A, chrom_gamma=chrom_gamma) or None
        cp_prior = _cproc.make_prior(len(self._cproc or []), cp_log10_A=cp_log10_A, cp_gamma=cp_gamma) or None
        prior = None   # (white-noise or chromatic boxes alone are a prior; nothing at all is _hyper.make_prior's "no parameter given")
        if (wn_prior is None and chrom_prior is None and cp_prior is None) or any(x is not None for x in (gwb_log10_A, gwb_gamma, rn_log10_A, rn_gamma, gwb_log10_hc, gwb_clm)):
            prior = _hyper.make_prior(self.P, _hyper._n_nodes(self._gw), _hyper.n_lm(self._gw), gwb_log10_A=gwb_log10_A, gwb_gamma=gwb_gamma,
                                      rn_log10_A=rn_log10_A, rn_gamma=rn_gamma, gwb_log10_hc=gwb_log10_hc, gwb_clm=gwb_clm)
        self._chrom_prior = chrom_prior
        self._cproc_prior = cp_prior
        self._prior, self._wn_prior = prior, wn_prior   # new dicts: the device copies of the previous boxes are not theirs (_uniform_table)
        return self

    def set_population(self, vals, number=None, fobs=None, T_obs=None, outlier_per_bin=100, population=None):
        """a binned binary population PER REALISATION (the reference's add_gwb_plus_outlier_cws, deterministic.py:565-715, with the
        Poisson sampling of the counts in front of it): vals [4, B] (Mtot, q, z, f_obs), number [B] >= 0 the expected count of every
        cell, fobs [F + 1] the bin edges, T_obs [s].  Realisation rho draws N_b ~ Poisson(number_b) (stream (11, attempt), pair = cell:
        csrc/pta_pop.h), forms w_b = ((N_b hs2_b) fo_b) T_obs, makes the outlier_per_bin <= 128 loudest cells of every bin (w > 0;
        ties: the lower cell index) CW sources and sums the rest into the free spectrum: population_theta().  Needs
        set_gwb(..., userSpec=U) with U[:, 0] = _population.f_centers(fobs) and set_cw(...); refused next to set_cw_prior and a
        gwb_log10_hc prior, which define the same keys, and in TD mode; F <= 64.  sample_theta / generate_sampled then include it.
        population: the holodeck-equivalent helpers (_population.Population).  set_population(None) removes it.  No prepare() needed."""
        if vals is None:
            self._pop = self._popd = None
            return self
        tab = _pop.make_tables(vals, number, fobs, T_obs, outlier_per_bin, population)
        _pop.check_engine(tab, self._gw, self._cw, getattr(self, "_cw_prior", None), getattr(self, "_prior", None),
                          getattr(self, "_td_prepared", False))
        self._pop, self._popd = tab, None   # _popd: the device copies, made by the first population_theta()
        return self

    def population_theta(self, R, r0=0, counts=None, raw=False):
        """theta of realisations r0 .. r0+R-1 of the population (set_population), made on chip by pta_pop_draw_select -> pta_pop_theta
        in batches bounded by workspace_bytes: {gwb_log10_hc [R, F], the cw_* source keys [R, S] with cw_log10_dist, S = F
        outlier_per_bin, bin-major, NaN past cw_count [R] (int32), pop_cell [R, S] (int32, -1 past the count), pop_number [R, S]}.  The
        orientation keys are pta_cw_catalog_uniform's, source s from stream (8, s).  counts [R, B]: the cell counts of every row (in
        the caller's cell order) instead of the Poisson draw - the reference's own `weights`.  raw=True adds the kernels' own
        outputs: pop_free_spec [R, F], pop_sel_w [R, F, k], pop_sel_count [R, F] and, without counts, pop_counts [R, B] (the drawn N;
        NaN for cells outside the bin edges) - for tests and measurements, not theta keys.  A row is a function of (seed, r0 + r)
        alone."""
        tab = getattr(self, "_pop", None)
        if tab is None:
            raise ValueError("population_theta: no population configured (set_population)")
        _pop.check_engine(tab, self._gw, self._cw, getattr(self, "_cw_prior", None), getattr(self, "_prior", None),
                          getattr(self, "_td_prepared", False))
        if counts is not None:
            counts = _pop.check_counts(counts, R, tab["B"])
        if self._popd is None:
            self._popd = population_device_tables(tab)
        S = tab["F"] * tab["k"]
        per_real = 20 * S + 12 * tab["F"]   # the selection scratch and the two [F] rows of one realisation, bytes
        step = int(max(1, min(R, self.workspace_bytes // per_real)))
        out = population_run(self._popd, self.seed, R, r0, counts=counts, raw=raw, step=step, scratch=self._scratch)
        prior = self._popd.setdefault("prior", _pop.orientation_prior(self.P, S))
        catalog = self._uniform_table("pta_cw_catalog_uniform", "pop", prior, lambda: _cw.prior_bounds(prior, self.P), R, r0, mid=(S,),
                                      shape=(R, S, _cw.N_SRC))
        theta = _cw.labels(None, prior, self.P, catalog)
        theta.update(out)
        return theta

    # ---------------------------------------------------------------- theta -> its parts --------
    def _theta_parts(self, theta, R, td=False, check_values=True):
        """(hyper, det): theta of R realisations split and validated before anything is launched.  hyper: its GWB / red-noise keys
        (_hyper.check_theta), None for the fixed-parameter path (no theta, or the keys of det alone); det: the keys whose terms are
        added after the fused launch, the CW keys (_cw.check_theta), the BWM keys (_bwm.check_theta), the wavelet burst and noise-transient keys (_burst.check_theta, check_nt_theta), the chromatic-event keys (_chrom_event.check_theta) and the white-noise keys
        (_wn_hyper.check_theta) and the chromatic keys (_chrom.check_theta) in one dict, {} if none.  td=True: TD mode, which takes deterministic keys only.  check_values=False
        skips the value checks (theta drawn by sample_theta)."""
        if theta is None:
            return None, {}
        if _hyper.ORF_INFO_KEY in theta:   # a label of sampled theta, no parameter
            theta = {k: v for k, v in theta.items() if k != _hyper.ORF_INFO_KEY}
        if isinstance(theta, dict):
            theta = _pop.strip_labels(theta)                  # and so are the population's pop_cell / pop_number
        rest, wnk = _wn_hyper.split(theta)   # ahead of _hyper.check_theta, whose key list stays the GWB / red-noise one
        rest, chk = _chrom.split(rest)
        rest, cpk = _cproc.split(rest)
        rest, cw = _cw.split(rest)
        rest, bwm = _bwm.split(rest)
        rest, bst, ntk = _burst.split(rest)
        rest, cek = _chrom_event.split(rest)
        if td:
            _chrom.refuse_td(self._chrom)
            _cproc.refuse_td(self._cproc)
            _wn_hyper.refuse_td(wnk)
        if td and (rest or not (cw or bwm or bst or ntk or cek)):   # a deterministic term leaves the factored covariance as it is
            raise ValueError("per-realisation theta is not supported in TD mode (the dense factors are built for one covariance; only "
                             "cw_*, bwm_*, burst_*, nt_* and ce_* keys are): use generate(theta=...) or generate_sampled()")
        det = dict(_cw.check_theta(cw, R, self.P, self._cw, check_values))
        det.update(_bwm.check_theta(bwm, R, self._bwm, check_values))
        det.update(_burst.check_theta(bst, R, getattr(self, "_burst", None), check_values))
        det.update(_burst.check_nt_theta(ntk, R, self.P, getattr(self, "_nt", None), check_values))
        det.update(_chrom_event.check_theta(cek, R, self.P, getattr(self, "_ce", None), check_values))
        det.update(_wn_hyper.check_theta(wnk, R, self.P, self._wn, self._ec, self.wn_mode, check_values))
        det.update(_chrom.check_theta(chk, R, self.P, self._chrom, check_values))
        det.update(_cproc.check_theta(cpk, R, self._cproc, check_values))
        if det and not rest:
            return None, det
        return _hyper.check_theta(rest, R, self.P, self._gw, self._rn, self.gwb_mode, check_values), det

    def _det_apply(self, det, R, out):
        """out[R, n_toa] += the deterministic terms of every row for the validated deterministic keys of theta (the second member of
        _theta_parts): the CW term, then the burst with memory, then the wavelet burst, then the noise transients, then the chromatic events."""
        if _cw.has_keys(det):
            self._cw_apply(det, R, out)
        if _bwm.has_keys(det):
            self._bwm_apply(det, R, out)
        if _burst.has_keys(det):
            self._burst_apply(det, R, out)
        if _burst.has_nt_keys(det):
            self._nt_apply(det, R, out)
        if _chrom_event.has_keys(det):
            self._ce_apply(det, R, out)
        return out

    # ---------------------------------------------------------------- what the terms share ------
    def _scratch(self, name, *shapes):
        """the reused device table(s) `name` of a term, float64, at least shapes[i][0] rows of exactly shapes[i][1:]: the cached ones
        while every one of them is large enough, else all of them are dropped first and allocated at `shapes` (one tensor for one
        shape, a tuple otherwise).  They stay outside the workspace budget."""
        tab = self._scratch_tabs.get(name)
        if tab is None or any(t.shape[0] < sh[0] or tuple(t.shape[1:]) != tuple(sh[1:]) for t, sh in zip(tab, shapes)):
            self._scratch_tabs[name] = None
            tab = self._scratch_tabs[name] = tuple(dv.empty(sh) for sh in shapes)
        return tab[0] if len(shapes) == 1 else tab

    def _term_batches(self, params, add, struct, rows, R, step, out, accumulate, draw=None):
        """out[R, n_toa] (+)= a term in batches of `step` realisations: per batch the entry `params` fills the tables of the filled
        ctypes struct, then the entry `add` walks the engine's tiles.  rows: [(field, tensor or None, bytes per row)], the members of
        the struct that follow the batch (None stays NULL).  draw = (seed, r0): `params` draws, and takes (seed, first realisation of the
        batch) behind the struct."""
        s = dv.stream_ptr()
        for lo in range(0, R, step):
            n = min(step, R - lo)
            for field, t, nbytes in rows:
                setattr(struct, field, None if t is None else t.data_ptr() + nbytes * lo)
            _lib.call(params, ctypes.byref(struct), *(() if draw is None else (draw[0], draw[1] + lo)), n, s)
            _lib.call(add, ctypes.byref(self.plan), ctypes.byref(struct), n, ctypes.c_void_p(out.data_ptr() + 8 * lo * out.stride(0)),
                      out.stride(0), 1 if accumulate else 0, s)
        return out

    def _phat_device(self):
        """pulsar unit vectors [P, 3] on the device (the reference's expression, deterministic.py:88, :858), built once."""
        if getattr(self, "_d_phat", None) is None:
            self._d_phat = dv.f64(_cw.pulsar_vectors([ra_dec(p) for p in self.psrs]))
        return self._d_phat

    def _cw_tables(self):
        """theta-independent device tables of the CW path: the pulsar unit vectors (_phat_device) and, built once per set_cw(), the
        configured pulsar distances [P] (kpc)."""
        if self._cwt is None:
            self._cwt = {"phat": self._phat_device(), "pdist": dv.f64(self._cw["pdist"])}
        return self._cwt

    # ---------------------------------------------------------------- CW, catalogue, BWM --------
    def _cw_apply(self, cw, R, out, accumulate=True):
        """out[R, n_toa] (+)= the CW term of every row for validated CW theta `cw` (row r = the source of realisation r0 + r): the
        source table -> pta_engine_cw_params -> pta_engine_cw_add, in batches of max_batch(hyper=True, cw=True).  Source keys of
        shape [R, S] are a catalogue (_cw_catalog_apply)."""
        if _cw.is_catalog(cw):
            return self._cw_catalog_apply(cw, R, out, accumulate)
        if not self._prepared:
            self.prepare()
        P = self.P
        amp = _cw.amp_key(cw)
        cols = [dv.as_f64(cw[amp if c == "amp" else "cw_" + c]).reshape(R, 1) for c in _cw.COLUMNS]
        has_pd = _cw.PDIST_KEY in cw
        if has_pd:
            cols.append(dv.as_f64(cw[_cw.PDIST_KEY]).reshape(R, P))
        src = torch.cat(cols, dim=1).contiguous()
        conf, tb = self._cw, self._cw_tables()
        step = min(R, self.max_batch(hyper=True, cw=True))
        c = _lib.CwEngine()
        c.n_psr, c.mode, c.psr_term, c.amp_is_h, c.has_pdist = P, _cw.mode(conf), int(conf["psrTerm"]), int(amp == "cw_log10_h"), int(has_pd)
        c.tref, c.phat, c.pdist, c.toa_s = conf["tref"], tb["phat"].data_ptr(), tb["pdist"].data_ptr(), self.d_toa_s.data_ptr()
        c.ld_src, c.par = src.stride(0), self._scratch("cw_par", (step, P, _lib.CW_ENGINE_NPAR)).data_ptr()
        self._term_batches("pta_engine_cw_params", "pta_engine_cw_add", c, [("src", src, 8 * src.stride(0))], R, step, out, accumulate)
        self._keep["cw"] = src   # the launches above read it asynchronously
        return out

    def _cw_catalog_apply(self, cw, R, out, accumulate=True):
        """out[R, n_toa] (+)= the sum of the catalogue of every row for validated CW theta `cw` with source keys [R, S] (and cw_count
        [R]): the [R, S, 8] source table -> pta_engine_cw_catalog_params -> pta_engine_cw_catalog_add (one accumulator per element over
        the sources, one read-modify-write of out), in batches of max_batch(hyper=True, cw=S)."""
        if not self._prepared:
            self.prepare()
        dev = dv.require_gpu()
        P, S = self.P, _cw.n_sources(cw)
        amp = _cw.amp_key(cw)
        src = torch.stack([dv.as_f64(cw[amp if c == "amp" else "cw_" + c]).reshape(R, S) for c in _cw.COLUMNS], dim=2).contiguous()   # [R, S, 8]
        has_pd = _cw.PDIST_KEY in cw
        conf, tb = self._cw, self._cw_tables()
        pdist = dv.as_f64(cw[_cw.PDIST_KEY]).reshape(R, P) if has_pd else tb["pdist"]
        count = cw.get(_cw.COUNT_KEY)
        if count is not None:
            count = (count.to(device=dev, dtype=torch.int32) if hasattr(count, "data_ptr") else dv.i32(count)).reshape(R).contiguous()
        mode = _cw.mode(conf)
        step = min(R, self.max_batch(hyper=True, cw=S))
        c = _lib.CwCatalogEngine()
        c.n_psr, c.n_src, c.mode, c.psr_term, c.amp_is_h, c.has_pdist = P, S, mode, int(conf["psrTerm"]), int(amp == "cw_log10_h"), int(has_pd)
        c.tref, c.phat, c.toa_s = conf["tref"], tb["phat"].data_ptr(), self.d_toa_s.data_ptr()
        c.ld_src, c.ld_pdist = src.stride(0), (pdist.stride(0) if has_pd else 0)
        c.par = self._scratch("cwc_par", (step * P * S * _lib.CW_CATALOG_NPAR[mode],)).data_ptr()
        rows = [("src", src, 8 * src.stride(0)), ("pdist", pdist, 8 * pdist.stride(0) if has_pd else 0), ("count", count, 4)]
        self._term_batches("pta_engine_cw_catalog_params", "pta_engine_cw_catalog_add", c, rows, R, step, out, accumulate)
        self._keep["cw"] = (src, pdist, count)   # the launches above read them asynchronously
        return out

    def _bwm_apply(self, det, R, out, accumulate=True):
        """out[R, n_toa] (+)= the burst-with-memory term of every row for validated theta `det` (row r = the burst of realisation
        r0 + r): the [R, 5] label table -> pta_engine_bwm_params (coef [R, P], t0 [R]) -> pta_engine_bwm_add, in batches of max_batch().
        The tables are R (P + 1) doubles and stay outside the workspace budget."""
        if not self._prepared:
            self.prepare()
        P = self.P
        src = torch.stack([dv.as_f64(det[k]).reshape(R) for k in _bwm.KEYS], dim=1).contiguous()   # [R, 5]
        step = min(R, self.max_batch())
        coef, t0 = self._scratch("bwm_tab", (step, P), (step,))
        b = _lib.BwmEngine()
        b.n_psr, b.phat, b.toa_s = P, self._phat_device().data_ptr(), self.d_toa_s.data_ptr()
        b.ld_src, b.coef, b.t0_s = src.stride(0), coef.data_ptr(), t0.data_ptr()
        self._term_batches("pta_engine_bwm_params", "pta_engine_bwm_add", b, [("src", src, 8 * src.stride(0))], R, step, out, accumulate)
        self._keep["bwm"] = src   # the launches above read it asynchronously
        return out

    # ---------------------------------------------------------------- wavelet burst, transients -
    def _count_device(self, count, R):
        """an optional count key of theta as a contiguous int32 device tensor [R]"""
        if count is None:
            return None
        return (count.to(device=dv.require_gpu(), dtype=torch.int32) if hasattr(count, "data_ptr") else dv.i32(np.asarray(count))).reshape(R).contiguous()

    def _burst_quad_tables(self):
        """theta-independent tables of remove_quad, built once per prepare(): the first TOA of every pulsar [P + 1] and the orthonormal
        basis of (1, t, t^2) over every pulsar's TOAs [n_toa, 3] (_burst.quad_basis)"""
        if getattr(self, "_burst_quad", None) is None or self._burst_quad[0] is not self.d_toa_s:
            self._burst_quad = (self.d_toa_s, dv.i32(np.asarray(self.off, dtype=np.int32)), dv.f64(_burst.quad_basis([m * 86400 for m in self.mjd])))
        return self._burst_quad[1:]

    def _burst_apply(self, det, R, out, accumulate=True):
        """out[R, n_toa] (+)= the wavelet burst of every row for validated theta `det`: the sky [R, 3] and wavelet [R, W, 7] label
        tables -> pta_engine_burst_params (wav [R, W, 7], kk [R, P, 2]) -> pta_engine_burst_add (with remove_quad: pta_engine_burst_quad,
        c [R, P, 3], inside it), in batches of max_batch() bounded by the one-launch index range of the tables.  The tables are
        R (7 W + 2 P (+ 3 P)) doubles and stay outside the workspace budget."""
        if not self._prepared:
            self.prepare()
        P, W, quad = self.P, self._burst["W"], self._burst["remove_quad"]
        sky = torch.stack([dv.as_f64(det[k]).reshape(R) for k in _burst.SKY_KEYS], dim=1).contiguous()      # [R, 3]
        src = torch.stack([dv.as_f64(det[k]).reshape(R, W) for k in _burst.WAV_KEYS], dim=2).contiguous()   # [R, W, 7]
        count = self._count_device(det.get(_burst.COUNT_KEY), R)
        step = min(R, self.max_batch(), 65535, ((1 << 31) - 1) // (max(7 * W, 3 * P) + W + P))
        wav, kk, qc = self._scratch("burst_tab", (step, W, 7), (step, P, 2), (step if quad else 0, P, 3))
        b = _lib.BurstEngine()
        b.n_psr, b.n_wav, b.phat, b.toa_s = P, W, self._phat_device().data_ptr(), self.d_toa_s.data_ptr()
        b.wav, b.kk = wav.data_ptr(), kk.data_ptr()
        if quad:
            off, q = self._burst_quad_tables()
            b.psr_off, b.quad_q, b.quad_c = off.data_ptr(), q.data_ptr(), qc.data_ptr()
        rows = [("sky", sky, 8 * 3), ("src", src, 8 * 7 * W), ("count", count, 4)]
        self._term_batches("pta_engine_burst_params", "pta_engine_burst_add", b, rows, R, step, out, accumulate)
        self._keep["burst"] = (sky, src, count)   # the launches above read them asynchronously
        return out

    def _nt_apply(self, det, R, out, accumulate=True):
        """out[R, n_toa] (+)= the noise transients of every row for validated theta `det`: the [R, V, 6] label table ->
        pta_engine_transient_params (tab [R, V, 6]) -> pta_engine_transient_add, in batches of max_batch()."""
        if not self._prepared:
            self.prepare()
        V = self._nt["V"]
        src = torch.stack([dv.as_f64(det[k]).reshape(R, V) for k in _burst.NT_KEYS], dim=2).contiguous()   # [R, V, 6]
        count = self._count_device(det.get(_burst.NT_COUNT_KEY), R)
        step = min(R, self.max_batch(), ((1 << 31) - 1) // (7 * V))
        t = _lib.TransientEngine()
        t.n_psr, t.n_wav, t.toa_s = self.P, V, self.d_toa_s.data_ptr()
        t.tab = self._scratch("nt_tab", (step, V, 6)).data_ptr()
        rows = [("src", src, 8 * 6 * V), ("count", count, 4)]
        self._term_batches("pta_engine_transient_params", "pta_engine_transient_add", t, rows, R, step, out, accumulate)
        self._keep["transient"] = (src, count)   # the launches above read them asynchronously
        return out

    # ---------------------------------------------------------------- chromatic events ----------
    def _ce_lnu_device(self):
        """lnu [n_toa] = ln(nu_ref / nu_i) over the concatenated TOAs on the device, tabulated in long double and rounded to float64 once
        per prepare() (_chrom_event.log_freq_ratio)"""
        if getattr(self, "_ce_lnu", None) is None or self._ce_lnu[0] is not self.d_toa_s:
            lnu = [_chrom_event.log_freq_ratio(_chrom.toa_freqs(p), self._ce["ref_freq_mhz"], name=f"pulsar {getattr(p, 'name', '?')}")
                   for p in self.psrs]
            self._ce_lnu = (self.d_toa_s, dv.f64(np.concatenate(lnu)))
        return self._ce_lnu[1]

    def _ce_apply(self, det, R, out, accumulate=True):
        """out[R, n_toa] (+)= the chromatic events of every row for validated theta `det`: the [R, E, 9] label table ->
        pta_engine_chrom_event_params (tab [R, E, 10]) -> pta_engine_chrom_event_add, in batches of max_batch()."""
        if not self._prepared:
            self.prepare()
        E = self._ce["E"]
        src = torch.stack([dv.as_f64(det[k]).reshape(R, E) for k in _chrom_event.KEYS], dim=2).contiguous()   # [R, E, 9]
        count = self._count_device(det.get(_chrom_event.COUNT_KEY), R)
        step = min(R, self.max_batch(), ((1 << 31) - 1) // (11 * E))
        c = _lib.ChromEventEngine()
        c.n_psr, c.n_ev, c.toa_s, c.lnu = self.P, E, self.d_toa_s.data_ptr(), self._ce_lnu_device().data_ptr()
        c.tab = self._scratch("ce_tab", (step, E, 10)).data_ptr()
        rows = [("src", src, 8 * 9 * E), ("count", count, 4)]
        self._term_batches("pta_engine_chrom_event_params", "pta_engine_chrom_event_add", c, rows, R, step, out, accumulate)
        self._keep["chrom_event"] = (src, count)   # the launches above read them asynchronously
        return out

    # ---------------------------------------------------------------- chromatic process ---------
    def _chrom_theta_device(self, det, R):
        """validated chromatic keys of theta -> (log10_A, gamma) contiguous float64 device tensors [R, P], a key not given filled with
        the configured values, pulsars configured without the process NaN amplitudes (they keep none); (None, None) without keys"""
        if not _chrom.has_keys(det):
            return None, None
        conf = _chrom.configured(self._chrom)
        lA, g = (dv.as_f64(det[k]) if k in det else dv.f64(np.ascontiguousarray(np.broadcast_to(c, (R, self.P))))
                 for k, c in zip(_chrom.KEYS, conf))
        none = np.flatnonzero(np.isnan(conf[0]))
        if len(none) and _chrom.A_KEY in det:
            lA = lA.clone()
            lA[:, dv.i64(none)] = float("nan")
        return lA, g

    def _chrom_apply(self, det, R, r0, out, accumulate=True):
        """out[R, n_toa] (+)= the chromatic term of realisations r0 .. r0+R-1 (row r = realisation r0 + r), with theta's chrom_* keys
        of `det` where it has them: pta_engine_chrom_coef (coef [n, P, K_c], drawn from stream (10, pulsar)) -> pta_engine_chrom_add, in
        batches of max_batch().  The coefficient table stays outside the workspace budget."""
        if not self._prepared:
            self.prepare()
        t = self._chrom_t
        P, Kc = self.P, t["K"]
        lA, g = self._chrom_theta_device(det, R)
        step = min(R, self.max_batch())
        c = _lib.ChromEngine()
        c.n_psr, c.k, c.rng_fast = P, Kc, int(self.rng_fast)
        c.Ft, c.ldf, c.amp, c.f, c.tspan = t["Ft"].data_ptr(), t["Ft"].stride(0), t["amp"].data_ptr(), t["f"].data_ptr(), t["tspan"].data_ptr()
        c.ld_theta = P
        c.coef = self._scratch("chrom_coef", (step, P, Kc)).data_ptr()
        rows = [("log10_A", lA, 8 * P), ("gamma", g, 8 * P)]
        self._term_batches("pta_engine_chrom_coef", "pta_engine_chrom_add", c, rows, R, step, out, accumulate, draw=(self.seed, r0))
        self._keep["chrom"] = (lA, g)   # the launches above read them asynchronously
        return out

    # ---------------------------------------------------------------- common processes ----------
    def _cproc_theta_device(self, det, R):
        """validated cp_* keys of theta -> (log10_A, gamma) contiguous float64 device tensors [R, n_proc], a key not given filled with
        the configured values; (None, None) without keys"""
        if not _cproc.has_keys(det):
            return None, None
        n = len(self._cproc)
        return tuple(dv.as_f64(det[k]) if k in det else dv.f64(np.ascontiguousarray(np.broadcast_to(c, (R, n))))
                     for k, c in zip(_cproc.KEYS, _cproc.configured(self._cproc)))

    def _cproc_struct(self):
        """pta_cproc_engine of the prepared tables, the per-batch members (log10_A, gamma, coef) left NULL"""
        t = self._cproc_t
        c = _lib.CprocEngine()
        c.n_psr, c.n_proc, c.k, c.rng_fast = self.P, len(t["kp"]), t["K"], int(self.rng_fast)
        for p, (kp, rho, B) in enumerate(zip(t["kp"], t["rho"], t["B"])):
            c.kp[p], c.rho[p], c.B[p] = kp, rho, B.data_ptr()
        c.amp, c.tspan, c.sc1, c.ld_theta = t["amp"].data_ptr(), t["T"], t["sc1"].data_ptr(), len(t["kp"])
        return c

    def _cproc_apply(self, det, R, r0, out, accumulate=True):
        """out[R, n_toa] (+)= the sum of the common processes of realisations r0 .. r0+R-1 (row r = realisation r0 + r), with theta's
        cp_* keys of `det` where it has them: pta_engine_cproc_coef (coef [n, P, K], drawn from stream (12, process)) ->
        pta_engine_cproc_add, in batches of max_batch().  The coefficient table stays outside the workspace budget."""
        if not self._prepared:
            self.prepare()
        n_proc = len(self._cproc)
        lA, g = self._cproc_theta_device(det, R)
        step = min(R, self.max_batch())
        c = self._cproc_struct()
        c.coef = self._scratch("cproc_coef", (step, self.P, self._cproc_t["K"])).data_ptr()
        rows = [("log10_A", lA, 8 * n_proc), ("gamma", g, 8 * n_proc)]
        self._term_batches("pta_engine_cproc_coef", "pta_engine_cproc_add", c, rows, R, step, out, accumulate, draw=(self.seed, r0))
        self._keep["cproc"] = (lA, g)   # the launches above read them asynchronously
        return out

    def _cproc_add_coef(self, coef, R, out, accumulate=False):
        """out[R, n_toa] (+)= the synthesis of given coefficients coef [R, P, K] (device): pta_engine_cproc_add alone (replay)"""
        c = self._cproc_struct()
        c.coef = coef.data_ptr()
        _lib.call("pta_engine_cproc_add", ctypes.byref(self.plan), ctypes.byref(c), R, ctypes.c_void_p(out.data_ptr()), out.stride(0),
                  1 if accumulate else 0, dv.stream_ptr())
        self._keep["cproc_coef"] = coef
        return out

    # ---------------------------------------------------------------- white noise ---------------
    def _wn_tables(self):
        """theta-independent device tables of the per-realisation white noise, built once per prepare(): sigma [n_toa], the white-noise
        group of every TOA and the ECORR group of every TOA's epoch (an epoch's flag is its first TOA's; -1 = in no group), the first
        group of every pulsar, and the configured efac / equad [s] / ecorr [s] of every group as prepare() computed them."""
        if self._wnh is not None:
            return self._wnh
        P, N = self.P, self.n_toa

        def flags_of(conf, a, idx):
            """flag values of TOAs idx of pulsar a; a pulsar that is its own group (flags None) reads no flags"""
            if _wn_hyper._pick_flags(conf["flags"], a, P) is None:
                return np.zeros(len(idx))
            return self._flag_array(a, conf["flagid"])[idx]
        t = {"sigma": dv.f64(np.concatenate(self.sigma_s)), "n_wn": 0, "n_ec": 0, "tnequad": 0, "max_per_psr": 1}
        if self._wn is not None:
            groups = self.wn_groups
            grp = np.concatenate([_wn_hyper.toa_groups(groups, a, flags_of(self._wn, a, np.arange(int(self.counts[a])))) for a in range(P)])
            efac, equad = _wn_hyper.configured_wn(P, self._wn)
            psr0 = _wn_hyper.psr_offsets(P, groups)
            t.update(n_wn=len(groups), wn_group=dv.i32(grp), wn_psr0=dv.i32(psr0), efac_conf=dv.f64(efac), equad_conf=dv.f64(equad),
                     tnequad=int(self._wn["tnequad"]))
            t["max_per_psr"] = max(t["max_per_psr"], int(np.diff(psr0).max()))
        if self._ec is not None and self.ecorr_groups:
            groups = self.ecorr_groups
            grp = np.full(N, -1, dtype=np.int32)
            for a in range(P):   # an epoch's flag is its first TOA's (white_noise.py:35)
                of_epoch = _wn_hyper.toa_groups(groups, a, flags_of(self._ec, a, self.epoch_first[a]))
                grp[self.off[a]:self.off[a + 1]] = of_epoch[self.epoch_of[a]]
            psr0 = _wn_hyper.psr_offsets(P, groups)
            t.update(n_ec=len(groups), ec_group=dv.i32(grp), ec_psr0=dv.i32(psr0), ecorr_conf=dv.f64(_wn_hyper.configured_ecorr(P, self._ec)))
            t["max_per_psr"] = max(t["max_per_psr"], int(np.diff(psr0).max()))
        self._wnh = t
        return t

    def _wn_theta_device(self, det, R):
        """validated white-noise keys of theta -> {"efac", "equad", "log10_ecorr": contiguous float64 device tensor [R, G] or None (key
        not given: as configured), "wn", "ecorr": whether the EFAC / EQUAD term and the ECORR term have a key}"""
        get = lambda k: dv.as_f64(det[k]) if k in det else None   # noqa: E731
        return {"efac": get(_wn_hyper.EFAC_KEY), "equad": get(_wn_hyper.EQUAD_KEY), "log10_ecorr": get(_wn_hyper.ECORR_KEY),
                "wn": _wn_hyper.has_wn(det), "ecorr": _wn_hyper.has_ecorr(det)}

    def _wn_add(self, wdev, lo, n, r_first, optr, ld_out, accumulate=True, wn=True, ecorr=True):
        """rows lo .. lo+n-1 of theta's white-noise labels `wdev` (_wn_theta_device) -> pta_engine_wn_params (the amplitude tables ea, eb
        [n, G_wn], ec [n, G_ec]) -> pta_engine_wn_add into the n rows at optr (realisations r_first ..): the EFAC / EQUAD term where
        theta has one of its keys (and wn), the ECORR term where it has that key (and ecorr); accumulate=False writes the terms alone
        (generate_per_signal).  The tables are n (2 G_wn + G_ec) doubles and stay outside the workspace budget, like the BWM tables."""
        w = self._wn_struct(wdev, lo, n, wn, ecorr)
        if w is None:
            return
        s = dv.stream_ptr()
        _lib.call("pta_engine_wn_params", ctypes.byref(w), n, s)
        _lib.call("pta_engine_wn_add", ctypes.byref(self.plan), ctypes.byref(w), self.seed, r_first, n, optr, ld_out, 1 if accumulate else 0, s)

    def _wn_struct(self, wdev, lo, n, wn=True, ecorr=True):
        """the pta_engine_wn_hyper of rows lo .. lo+n-1 of `wdev` with the terms asked for that theta has a key of (None: neither);
        its amplitude tables are the engine's reused buffers, grown on demand"""
        t = self._wn_tables()
        wn, ecorr = wn and wdev["wn"], ecorr and wdev["ecorr"]
        if not (wn or ecorr):
            return None
        ea, eb, ec = self._scratch("wn_amp", (n, t["n_wn"]), (n, t["n_wn"]), (n, t["n_ec"]))
        w = _lib.WnHyper()
        w.n_psr, w.n_wn, w.n_ec, w.tnequad, w.max_per_psr = self.P, t["n_wn"], t["n_ec"], t["tnequad"], t["max_per_psr"]
        w.sigma = t["sigma"].data_ptr()
        if wn:
            w.wn_group, w.wn_psr0, w.efac_conf, w.equad_conf = (t[k].data_ptr() for k in ("wn_group", "wn_psr0", "efac_conf", "equad_conf"))
            for name, ld, key in (("efac", "ld_efac", "efac"), ("log10_equad", "ld_equad", "equad")):
                if wdev[key] is not None:
                    setattr(w, name, dv.row_ptr(wdev[key], lo))
                    setattr(w, ld, wdev[key].stride(0))
            w.ea, w.eb = ea.data_ptr(), eb.data_ptr()
        if ecorr:
            w.ec_group, w.ec_psr0, w.ecorr_conf = (t[k].data_ptr() for k in ("ec_group", "ec_psr0", "ecorr_conf"))
            w.log10_ecorr, w.ld_ecorr = dv.row_ptr(wdev["log10_ecorr"], lo), wdev["log10_ecorr"].stride(0)
            w.ec = ec.data_ptr()
        return w

    # ---------------------------------------------------------------- theta drawn on chip -------
    def sample_theta(self, R, r0=0):
        """theta of realisations r0 .. r0+R-1 under the current prior, drawn on chip (what generate_sampled uses).  With a gwb_clm
        prior also gwb_orf_info [R] int32 (pta_gwb_orf_factor's info of every drawn sky; generate() and the statistics skip the key)."""
        return self._sample_theta(R, r0, orf_info=True)

    def _orf_info_of(self, clm):
        """info [R] int32 of pta_gwb_orf_factor for clm [R, n_lm] on the device, factored batch by batch into a scratch buffer"""
        R, P = clm.shape[0], self.P
        step = min(R, self.max_batch(hyper=True, clm=True))
        scratch, info = dv.empty((step, P, P)), dv.zeros((R,), dtype=torch.int32)
        for lo in range(0, R, step):
            _lib.call("pta_gwb_orf_factor", dv.ptr(self.d_orf_basis), clm.shape[1], P, dv.row_ptr(clm, lo), clm.stride(0), min(step, R - lo),
                      dv.ptr(scratch), ctypes.c_void_p(info.data_ptr() + 4 * lo), dv.stream_ptr())
        torch.cuda.current_stream().synchronize()   # scratch dies with the call
        return info

    def _uniform_table(self, entry, name, prior, bounds, R, r0, mid=None, shape=None):
        """[R, n] table (or `shape`) of the uniform entry `entry` for realisations r0 .. r0+R-1: column j uniform in the box (lo[j],
        hi[j]) of bounds() -> (lo, hi).  The boxes `name` are uploaded once per prior object: the cache entry holds the prior dict it
        was built from, so a set_*_prior call, which replaces the dict, invalidates it.  mid: the entry's arguments between R and lo
        (default: the column count n)."""
        d_lo, d_hi = self._box_device(name, prior, bounds)
        table = dv.empty(shape or (R, d_lo.shape[0]))
        _lib.call(entry, self.seed, r0, R, *((d_lo.shape[0],) if mid is None else mid), dv.ptr(d_lo), dv.ptr(d_hi), dv.ptr(table), dv.stream_ptr())
        return table

    def _box_device(self, name, prior, bounds):
        """(lo, hi) of the boxes `name` on the device, uploaded once per prior object (_uniform_table)"""
        ent = self._boxes.get(name)
        if ent is None or ent[0] is not prior:
            ent = self._boxes[name] = (prior, [dv.f64(x) for x in bounds()])
        return ent[1]

    def _sample_theta(self, R, r0, orf_info):
        prior, cw_prior, bwm_prior = getattr(self, "_prior", None), getattr(self, "_cw_prior", None), getattr(self, "_bwm_prior", None)
        wn_prior, chrom_prior, cp_prior = getattr(self, "_wn_prior", None), getattr(self, "_chrom_prior", None), getattr(self, "_cproc_prior", None)
        pop = getattr(self, "_pop", None)
        burst_prior, nt_prior, ce_prior = getattr(self, "_burst_prior", None), getattr(self, "_nt_prior", None), getattr(self, "_ce_prior", None)
        if (prior is None and cw_prior is None and bwm_prior is None and wn_prior is None and chrom_prior is None and cp_prior is None and pop is None
                and burst_prior is None and nt_prior is None and ce_prior is None):
            raise ValueError("sample_theta: no prior (set_hyper_prior / set_cw_prior / set_bwm_prior first)")
        if not self._prepared:
            self.prepare()
        theta = {}
        if pop is not None:         # streams (11, attempt), pair = cell, and (8, s) for the orientations: whatever else is sampled
            theta.update(self.population_theta(R, r0))
        if bwm_prior is not None:   # stream (9, 0): pair j = label column j, whatever else is sampled
            theta.update(_bwm.labels(self._uniform_table("pta_bwm_uniform", "bwm", bwm_prior, lambda: _bwm.prior_bounds(bwm_prior), R, r0, mid=())))
        if burst_prior is not None:   # streams (13, 0) and (13, 1 + w): pair j = label column j, whatever else is sampled
            if getattr(self, "_burst", None) is None:
                raise ValueError("sample_theta: no per-realisation wavelet burst configured (set_burst)")
            W = self._burst["W"]
            sky, wav = dv.empty((R, 3)), dv.empty((R, W, 7))
            d_lo, d_hi = self._box_device("burst", burst_prior, lambda: _burst.prior_bounds(burst_prior))
            _lib.call("pta_burst_uniform", self.seed, r0, R, W, dv.ptr(d_lo), dv.ptr(d_hi), dv.ptr(sky), dv.ptr(wav), dv.stream_ptr())
            theta.update(_burst.labels(sky, wav))
        if nt_prior is not None:      # stream (14, v): pair j = label column j, whatever else is sampled
            if getattr(self, "_nt", None) is None:
                raise ValueError("sample_theta: no per-realisation noise transients configured (set_transients)")
            V = self._nt["V"]
            theta.update(_burst.nt_labels(self._uniform_table("pta_transient_uniform", "nt", nt_prior, lambda: _burst.nt_prior_bounds(nt_prior, self.P),
                                                              R, r0, mid=(V, self.P), shape=(R, V, 6))))
        if ce_prior is not None:      # stream (15, e): pair j = label column j of slot e, whatever else is sampled
            if getattr(self, "_ce", None) is None or len(ce_prior["kind"]) != self._ce["E"]:
                raise ValueError("sample_theta: the chromatic-event prior does not match the configured events (set_chromatic_events, "
                                 "then set_chromatic_event_prior)")
            E = self._ce["E"]
            theta.update(_chrom_event.labels(self._uniform_table("pta_chrom_event_uniform", "chrom_event", ce_prior,
                                                                 lambda: _chrom_event.prior_bounds(ce_prior), R, r0, mid=(E, self.P), shape=(R, E, 9))))
        if cw_prior is not None:    # stream (8, 0): pair j = label column j, whatever else is sampled
            S, cw_bounds = cw_prior["n_sources"], lambda: _cw.prior_bounds(cw_prior, self.P)
            table = catalog = None
            if S is None or "pdist" in cw_prior:   # (with a catalogue: for the pdist columns, pairs 8 .. 8 + P - 1 of stream (8, 0))
                table = self._uniform_table("pta_cw_uniform", "cw", cw_prior, cw_bounds, R, r0)
            if S is not None:                      # source s from stream (8, s), pair = label column
                catalog = self._uniform_table("pta_cw_catalog_uniform", "cw", cw_prior, cw_bounds, R, r0, mid=(S,), shape=(R, S, _cw.N_SRC))
            theta.update(_cw.labels(table, cw_prior, self.P, catalog))
        for k, box in (wn_prior or {}).items():   # streams (7, 3 .. 5): pair j = group j, whatever else is sampled
            n_groups = len(self.ecorr_groups if k == _wn_hyper.ECORR_KEY else self.wn_groups)
            if len(box[0]) != n_groups:
                raise ValueError(f"sample_theta: the {k} boxes are for {len(box[0])} groups but the engine now has {n_groups}: "
                                 "call set_hyper_prior again")
            theta[k] = self._uniform_table("pta_hyper_uniform_field", k, wn_prior, lambda: box, R, r0, mid=(len(box[0]), _wn_hyper.FIELD[k]))
        if chrom_prior is not None and self._chrom is None:
            raise ValueError("sample_theta: chromatic boxes given but no chromatic process is configured (set_chromatic_noise)")
        for k, box in (chrom_prior or {}).items():   # streams (7, 6 .. 7): pair = pulsar, whatever else is sampled
            theta[k] = self._uniform_table("pta_hyper_uniform_field", k, chrom_prior, lambda: box, R, r0, mid=(self.P, _chrom.FIELD[k]))
            none = np.flatnonzero(np.isnan(_chrom.configured(self._chrom)[0]))
            if len(none):   # pulsars configured without the process keep none: their labels are NaN
                theta[k][:, dv.i64(none)] = float("nan")
        if cp_prior is not None and not self._cproc:
            raise ValueError("sample_theta: common-process boxes given but no common process is configured (add_common_process)")
        for k, box in (cp_prior or {}).items():   # streams (7, 8 .. 9): pair = process, whatever else is sampled
            if len(box[0]) != len(self._cproc):
                raise ValueError(f"sample_theta: the {k} boxes are for {len(box[0])} processes but the engine now has {len(self._cproc)}: "
                                 "call set_hyper_prior again")
            theta[k] = self._uniform_table("pta_hyper_uniform_field", k, cp_prior, lambda: box, R, r0, mid=(len(box[0]), _cproc.FIELD[k]))
        if prior is None:
            return theta
        box = _hyper.spec_bounds(prior)
        if box is not None:        # stream (7, 1): pair j = node j of the userSpec as given
            theta[_hyper.SPEC_KEY] = self._uniform_table("pta_hyper_uniform_field", "spec", prior, lambda: box, R, r0, mid=(len(box[0]), _hyper.SPEC_FIELD))
        box = _hyper.clm_bounds(prior, self._gw)
        if box is not None:        # stream (7, 2): pair j = column j of gwb_clm (column 0: the configured c_00)
            clm = theta[_hyper.CLM_KEY] = self._uniform_table("pta_hyper_uniform_field", "clm", prior, lambda: box, R, r0,
                                                              mid=(len(box[0]), _hyper.CLM_FIELD))
            if orf_info:
                theta[_hyper.ORF_INFO_KEY] = self._orf_info_of(clm)
        if not any(k in prior for k in _hyper.KEYS):
            return theta
        table = self._uniform_table("pta_hyper_uniform", "hyper", prior, lambda: _hyper.prior_bounds(prior, self.P), R, r0)
        cols = _hyper.columns(self.P)
        for k in _hyper.KEYS:
            if k in prior:
                c0, c1 = cols[k]
                theta[k] = table[:, c0].contiguous() if k in _hyper.GWB_KEYS else table[:, c0:c1].contiguous()
        if self.plan.rn_k:
            none = self._hyper_tables()["rn_none"]
            for k in _hyper.RN_KEYS:
                if k in theta and len(none):   # pulsars configured without red noise keep none: their labels are NaN
                    theta[k][:, none] = float("nan")
        return theta


# ---------------------------------------------------------------- population: device tables and the batch loop -----------------------
def population_device_tables(tab):
    """the host tables of _pop.make_tables on the device and the pta_pop_plan that points at them"""
    d = {k: (dv.i32 if k in ("cell_ptr", "orig") else dv.f64)(tab[k])
         for k in ("cell_ptr", "number", "hs2", "fo", "orig", "log10_mc", "log10_fo", "log10_dl")}
    p = _lib.PopPlan()
    p.n_cells, p.n_sorted, p.n_bins, p.k, p.t_obs = tab["B"], len(tab["orig"]), tab["F"], tab["k"], tab["T_obs"]
    for k, t in d.items():
        setattr(p, k, t.data_ptr())
    d["plan"] = p
    return d


def population_run(d, seed, R, r0=0, counts=None, raw=False, step=None, scratch=None):
    """pta_pop_draw_select -> pta_pop_theta for realisations r0 .. r0+R-1 in batches of `step` over the device tables d
    (population_device_tables): {gwb_log10_hc [R, F], cw_log10_mc, cw_log10_fgw, cw_log10_dist, pop_number [R, S], pop_cell [R, S] int32,
    cw_count [R] int32}; raw=True adds pop_free_spec, pop_sel_w, pop_sel_count and (drawn counts) pop_counts.  counts: [R, B] NumPy
    array or tensor, or None to draw.  scratch: the engine's _scratch (the selection tables are reused across calls); None allocates."""
    dev = dv.require_gpu()
    p = d["plan"]
    B, F, k = p.n_cells, p.n_bins, p.k
    S = F * k
    step = R if step is None else max(1, min(int(step), R))
    n_sel = step * S
    words = 2 * n_sel + (n_sel + 1) // 2   # sel_number, sel_w (float64) and sel_cell (int32) of one batch
    buf = dv.empty((words,)) if scratch is None else scratch("pop_sel", (words,))
    sel_number, sel_w, sel_cell = buf[:n_sel], buf[n_sel:2 * n_sel], buf[2 * n_sel:].view(torch.int32)
    f64 = lambda *sh: dv.empty(sh)   # noqa: E731
    out = {_hyper.SPEC_KEY: f64(R, F), "cw_log10_mc": f64(R, S), "cw_log10_fgw": f64(R, S), "cw_log10_dist": f64(R, S),
           _cw.COUNT_KEY: dv.empty((R,), dtype=torch.int32), "pop_cell": dv.empty((R, S), dtype=torch.int32), "pop_number": f64(R, S)}
    free_spec, sel_count = f64(R, F), dv.empty((R, F), dtype=torch.int32)
    if counts is not None:
        counts = (counts.to(device=dev, dtype=torch.float64) if hasattr(counts, "data_ptr") else dv.f64(counts)).contiguous()
    counts_out = torch.full((R, B), float("nan"), dtype=torch.float64, device=dev) if raw and counts is None else None
    all_w = dv.zeros((R, F, k)) if raw else None
    s = dv.stream_ptr()
    for lo in range(0, R, step):
        n = min(step, R - lo)
        _lib.call("pta_pop_draw_select", ctypes.byref(p), seed, r0 + lo, n, dv.row_ptr(counts, lo), B, dv.row_ptr(counts_out, lo), B,
                  dv.ptr(sel_cell), dv.ptr(sel_number), dv.ptr(sel_w), dv.row_ptr(sel_count, lo), dv.row_ptr(free_spec, lo), s)
        _lib.call("pta_pop_theta", ctypes.byref(p), n, dv.ptr(sel_cell), dv.ptr(sel_number), dv.row_ptr(sel_count, lo), dv.row_ptr(free_spec, lo),
                  dv.row_ptr(out["cw_log10_mc"], lo), dv.row_ptr(out["cw_log10_fgw"], lo), dv.row_ptr(out["cw_log10_dist"], lo),
                  dv.row_ptr(out["pop_number"], lo), dv.row_ptr(out["pop_cell"], lo), dv.row_ptr(out[_cw.COUNT_KEY], lo),
                  dv.row_ptr(out[_hyper.SPEC_KEY], lo), F, s)
        if raw:   # entries at or past sel_count are whatever the scratch held: masked below
            all_w[lo:lo + n] = sel_w[:n * S].view(n, F, k)
    if raw:
        live = torch.arange(k, device=dev)[None, None, :] < sel_count[:, :, None]
        out.update(pop_free_spec=free_spec, pop_sel_w=torch.where(live, all_w, torch.zeros_like(all_w)), pop_sel_count=sel_count)
        if counts_out is not None:
            out["pop_counts"] = counts_out
    return out
