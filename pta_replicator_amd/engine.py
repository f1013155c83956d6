"""ReplicaEngine: R independent realisations of a whole pulsar-timing array per call, on one MI355X.

The reference produces one realisation per sequence of ``add_*`` calls (a Python loop over pulsars, one pass
through PINT per call).  For ensembles the realisation-independent work - Fourier design matrices
(red_noise.py:36-103), epoch maps (white_noise.py:7-44), ORF + Cholesky (red_noise.py:200-235), spectrum
(:243-265), the DFT twiddle matrix, interpolation brackets (:286-287), CGW waveforms (deterministic.py:13-185) -
is done once in ``prepare()``; ``generate()`` then runs three kernels per batch:

  pta_engine_rn_coef   60 red-noise coefficients per (realisation, pulsar)
  pta_gwb_idft_rng     pruned inverse DFT of on-chip draws, fp64 MFMA      + pta_gwb_mix (ORF mix, MFMA)
  pta_engine_synth     fused RN + GWB-interp + EFAC/EQUAD + ECORR + deterministic -> out[R, sum N_a]

Draws are counter-based (Philox-4x32-10 keyed by seed; counter = pair, stream, realisation), so realisation r
is the same numbers whatever the batch size, launch geometry or number of GPUs.  ``replay()`` pushes
caller-supplied draws (e.g. NumPy's legacy stream in the reference's order, or ``dump_draws()``) through the
per-signal kernels - that is the parity path.

Realisations are defined on the IDEAL TOAs.  The reference applies each signal's delay to the TOAs before the
next ``add_*`` reads them (adjust_TOAs in every function); the induced difference is O(delay * f) ~ 1e-12
relative (SURVEY.md §7 "hard parts" ii) and is the stated tolerance floor of batched-vs-sequential parity.
"""
import ctypes

import numpy as np
import torch

from . import _burst, _bwm, _chrom, _chrom_event, _cproc, _cw, _hyper, _lib, _wn_hyper, device as dv
from . import deterministic as det
from . import red_noise as rn
from . import spharmORFbasis as anis
from . import white_noise as wn
from ._position import ra_dec
from .constants import DAY_IN_SEC, YEAR_IN_SEC
from .engine_bwm import BwmStatisticMixin
from .engine_clnl import CorrelatedLikelihoodMixin
from .engine_fstat import FStatisticMixin
from .engine_lnl import LikelihoodMixin
from .engine_os import OptimalStatisticMixin
from .engine_td import TimeDomainMixin
from .engine_terms import PerRealisationTermsMixin

STREAM_GWB, STREAM_RN, STREAM_WN, STREAM_ECORR, STREAM_TD, STREAM_TDGW = 1, 2, 3, 4, 5, 6
STREAM_HYPER = 7   # per-realisation hyperparameters (generate_sampled): stream_id(7, 0), pair = parameter column (_hyper.columns);
                   # stream_id(7, 1), pair = node: the per-realisation GWB spectrum (_hyper.SPEC_KEY);
                   # stream_id(7, 2), pair = column: the per-realisation angular power coefficients (_hyper.CLM_KEY);
                   # stream_id(7, 3 .. 5), pair = group: the per-realisation EFAC, log10 EQUAD and log10 ECORR (_wn_hyper.FIELD)
STREAM_CW = 8      # per-realisation CW source labels (generate_sampled): stream_id(8, 0), pair = label column (_cw.COLUMNS)
STREAM_BWM = 9     # per-realisation burst-with-memory labels (generate_sampled): stream_id(9, 0), pair = label column (_bwm.COLUMNS)
STREAM_CHROM = _chrom.STREAM_CHROM   # 10: the chromatic process, stream_id(10, pulsar), pair c >> 1, branch c & 1 = coefficient c (as STREAM_RN);
                                     # its prior boxes: stream_id(7, 6 .. 7), pair = pulsar (_chrom.FIELD)
STREAM_CPROC = _cproc.STREAM_CPROC   # 12: the common processes, stream_id(12, process), deviate n = c rho + j: pair n >> 1, branch n & 1;
                                     # their prior boxes: stream_id(7, 8 .. 9), pair = process (_cproc.FIELD).  (11: the population, _pop)


def stream_id(kind, pulsar):
    return ((kind << 24) | (pulsar & 0xFFFFFF)) & 0xFFFFFFFF


class ReplicaEngine(PerRealisationTermsMixin, TimeDomainMixin, OptimalStatisticMixin, LikelihoodMixin, CorrelatedLikelihoodMixin, FStatisticMixin,
                    BwmStatisticMixin):
    def __init__(self, psrs, seed=0):
        # pulsars with the reference's SimulatedPulsar surface are used as they are; enterprise-style ones (toas [s] / toaerrs [s] /
        # flags / pos as plain arrays: what simulate.py:91-95 hands on) are wrapped once through simulate.from_enterprise
        from .simulate import as_simulated
        self.psrs = [as_simulated(p) for p in psrs]
        self.P = len(self.psrs)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.names = [p.name for p in self.psrs]
        # ideal TOAs: float64 MJD (GWB/ECORR/CGW read get_mjds, red_noise.py:287, white_noise.py:158,
        # deterministic.py:98) and float64(tdbld)*86400 (RN, red_noise.py:123)
        self.mjd = [np.asarray(p.toas.get_mjds().value, dtype=np.float64) for p in self.psrs]
        self.tdb_s = [np.array(p.toas.table["tdbld"], dtype="float64") * DAY_IN_SEC for p in self.psrs]
        self.sigma_s = [np.asarray(p.toas.get_errors().to("s").value, dtype=np.float64) for p in self.psrs]
        self.counts = np.array([len(m) for m in self.mjd])
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.n_toa = int(self.off[-1])
        self._rn = None
        self._wn = None
        self._ec = None
        self._gw = None
        self._det = None
        self._delays = None
        self._cw = None      # one CW source per realisation (set_cw), parameters from theta / set_cw_prior
        self._bwm = False    # one burst with memory per realisation (set_bwm), parameters from theta / set_bwm_prior
        self._burst = None   # a burst of sine-Gaussian wavelets per realisation (set_burst), parameters from theta / set_burst_prior
        self._nt = None      # noise transients per realisation (set_transients), parameters from theta / set_transient_prior
        self._ce = None      # chromatic events per realisation (set_chromatic_events), parameters from theta / set_chromatic_event_prior
        self._pop = self._popd = None   # a binary population per realisation (set_population): host tables, their device copies
        self._chrom = None   # one chromatic Gaussian process per pulsar (set_chromatic_noise), added after the fused launch
        self._chrom_t = None   # its device tables, built by prepare()
        self._cproc = None   # up to four common red processes with an ORF each (add_common_process), added after the chromatic term
        self._cproc_t = None   # their device tables, built by prepare()
        # state of the per-realisation terms (engine_terms.py): per term the buffers its queued launches still read, replaced when the
        # term next runs; the reused device tables (_scratch); the device copies of the prior boxes (_uniform_table)
        self._keep, self._scratch_tabs, self._boxes = {}, {}, {}
        self._prepared = False
        # frequency -> time transform of the GWB in throughput mode: "auto" = chirp-z FFT when it fits, else the MFMA DFT-GEMM
        self.gwb_transform = "auto"
        # per-engine options, copied into the plan / tables structs of every call (the library has no process-wide switches)
        self.rng_fast = 0        # 1 = fp32-transcendental Gaussian transform (opt-in; all ranks of a job must agree)
        self.synth_variant = 0   # pta_engine_plan.synth_variant
        self.czt_variant = 0     # pta_engine_tables.czt_variant
        self.mix_variant = 0     # pta_engine_tables.mix_variant
        self.idft_variant = 1    # column tiling of the DFT-GEMM form; fixed at prepare() (the twiddle layout depends on it)
        # how the GWB of generate() is drawn: "fourier" (default) = the reference's 2 Nf complex-bin deviates per pulsar through
        # its frequency-domain synthesis (replayable through the reference algebra, dump_draws / replay); "grid" = npts deviates
        # per pulsar through the Cholesky factor of the covariance that synthesis implies on the npts-sample grid (SURVEY.md
        # App. A.1) - same distribution, 10x fewer deviates, the transform becomes an MFMA triangular product
        self.gwb_mode = "fourier"
        # how the EFAC/EQUAD term of generate() is drawn: "reference" (default) = two deviates per TOA, (efac sigma) z1 + (efac equad) z2,
        # the reference's own draws (white_noise.py:105-109: replayable, dump_draws / replay); "single" = ONE deviate per TOA with the
        # combined amplitude sqrt((efac sigma)^2 + (efac equad | equad)^2) - same distribution, half the Box-Muller pairs of the fused
        # kernel, not the reference's draw order (opt-in secondary number of bench.py, never `value`)
        self.wn_mode = "reference"
        self.workspace_bytes = 8 << 30   # upper bound of the per-batch workspace of generate() (cap by bytes, not only by count)

    # ---------------------------------------------------------------- configuration -------------
    def set_red_noise(self, log10_amplitude, spectral_index, components=30, libstempo_convention=False):
        """per-pulsar power-law red noise; entries may be None to skip a pulsar (red_noise.py:106-135)."""
        self._rn = dict(A=list(np.broadcast_to(np.asarray(log10_amplitude, dtype=object), (self.P,))),
                        g=list(np.broadcast_to(np.asarray(spectral_index, dtype=object), (self.P,))),
                        components=int(components), libstempo=bool(libstempo_convention))
        self._prepared = False

    def set_chromatic_noise(self, log10_amplitude, spectral_index, components=30, index=2.0, ref_freq_mhz=1400.0):
        """one chromatic power-law Gaussian process per pulsar, dt_i = (ref_freq_mhz / nu_i)^index sum_k F_ik sqrt(phi_k) z_k with the
        basis and prior of the red noise (red_noise.py:106-128) and `components` frequencies of its own: index 2 = DM variations.
        Amplitude and spectral index per pulsar as in set_red_noise (a scalar or a list; None = no process for that pulsar).  The
        radio frequencies come from the pulsars (toas.freqs_mhz, else toas.get_freqs()).  Drawn from stream (10, pulsar) and added
        after the fused launch (pta_engine_chrom_coef -> pta_engine_chrom_add); theta's chrom_log10_A / chrom_gamma [R, P] give it
        parameters per realisation (_chrom).  Not available in TD mode, nor under the theta-matched OS and the likelihood."""
        self._chrom = _chrom.make_config(self.P, log10_amplitude, spectral_index, components, index, ref_freq_mhz)
        self._prepared = False

    def add_common_process(self, log10_amplitude, spectral_index, orf="curn", components=14):
        """one more common power-law Gaussian process (at most four) with an ORF of its own: "hd", "monopole" (a clock error), "dipole"
        (an ephemeris error), "curn" (no correlations) or a symmetric positive semi-definite [P, P] array.  On the array-wide basis
        f_k = k / T, k <= components <= 32 (T = the span of the whole array; the basis the likelihoods and the OS model a common
        process on), dt_{a,i} += sum_c F_ic sqrt(phi_c) sum_j B[a, j] z_cj with B B^T = the ORF and phi the red-noise prior at
        Tspan = T.  Drawn from stream (12, process) and added after the fused launch and the chromatic term (pta_engine_cproc_coef ->
        pta_engine_cproc_add); theta's cp_log10_A / cp_gamma [R, n_proc] give the processes parameters per realisation (_cproc).  Works
        with or without set_gwb and for a single pulsar.  Not available in TD mode, nor under the theta-matched OS and the likelihood."""
        proc = _cproc.make_process(self._unit_vectors(), log10_amplitude, spectral_index, orf, components)
        self._cproc = _cproc.add(self._cproc, proc)
        self._prepared = False
        return self

    @property
    def common_processes(self):
        """the configured common processes, in the order of the calls: [{log10_amplitude, spectral_index, orf, components, rank}]"""
        return [dict(log10_amplitude=p["A"], spectral_index=p["g"], orf=p["orf"], components=p["components"], rank=p["B"].shape[1])
                for p in (self._cproc or [])]

    def _unit_vectors(self):
        """unit vectors [P, 3] of the pulsars from their right ascension and declination (the ORFs of the common processes and of
        prepare_correlated_likelihood)"""
        from ._position import ra_dec
        pos = []
        for p in self.psrs:
            ra, dec = ra_dec(p, default=(0.0, 0.0))
            pos.append([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])
        return np.array(pos)

    def _cproc_toas(self):
        """the times [s] of the array-wide basis, per pulsar: those of _stats_noise_model"""
        return [m * 86400.0 for m in self.mjd]

    def _prepare_cproc(self):
        """the tables of the common processes (self._cproc_t): two doubles per TOA (sin, cos)(2 pi frac(t / T)) evaluated in long double
        on the host, the ORF factors, and the configured amplitudes [n_proc, K]"""
        t = _cproc.host_tables(self._cproc, self._cproc_toas())
        t.update(sc1=dv.f64(t["sc1_host"]), amp=dv.f64(t["amp_host"]), B=[dv.f64(b) for b in t["B_host"]])
        self._cproc_t = t

    def _cproc_low_rank_host(self):
        """(F [P][N_a, K], phi [P][K]): the auto-term of every common process on the array-wide basis, sum_p Gamma_p,aa phi_p - the columns
        the fixed-noise statistics add to the low-rank part of C_a.  NumPy alone."""
        return _cproc.low_rank_host(self._cproc, self._cproc_toas())

    def set_white_noise(self, efac=1.0, log10_equad=None, flagid="f", flags=None, tnequad=False):
        """EFAC/EQUAD (white_noise.py:47-125).  Scalars, per-pulsar lists of scalars, or (with `flags`, a per-pulsar
        list of flag lists) per-pulsar lists of per-flag arrays."""
        self._wn = dict(efac=efac, log10_equad=log10_equad, flagid=flagid, flags=flags, tnequad=bool(tnequad))
        self._prepared = False

    def set_jitter(self, log10_ecorr, flagid="f", flags=None, coarsegrain=0.1):
        """ECORR (white_noise.py:128-198)."""
        self._ec = dict(log10_ecorr=log10_ecorr, flagid=flagid, flags=flags, coarsegrain=float(coarsegrain))
        self._prepared = False

    def set_gwb(self, log10_amplitude, spectral_index, no_correlations=False, turnover=False,
                clm=(np.sqrt(4.0 * np.pi),), lmax=0, f0=1e-9, beta=1, power=1, userSpec=None, npts=600, howml=10):
        """common GWB process (red_noise.py:138-298)."""
        self._gw = dict(A=log10_amplitude, g=spectral_index, no_correlations=no_correlations, turnover=turnover, clm=clm,
                        lmax=lmax, f0=f0, beta=beta, power=power, userSpec=userSpec, npts=npts, howml=howml)
        self._prepared = False

    def add_cgw(self, **kw):
        """a continuous-wave source shared by all pulsars (deterministic.py:13-185); same keyword arguments."""
        self._det = (self._det or []) + [kw]
        self._prepared = False

    def add_delays(self, delays):
        """any precomputed deterministic delay (seconds; one array per pulsar or one concatenated array), e.g. the
        ``added_signals_time`` entry left by add_burst / add_gw_memory / add_catalog_of_cws: added to every realisation."""
        d = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in delays]) if isinstance(delays, (list, tuple)) \
            else np.asarray(delays, dtype=np.float64).ravel()
        if d.shape != (self.n_toa,):
            raise ValueError("delays must cover all {} TOAs, got {}".format(self.n_toa, d.shape))
        self._delays = d if getattr(self, "_delays", None) is None else self._delays + d
        self._prepared = False

    # ---------------------------------------------------------------- helpers -------------------
    @property
    def wn_groups(self):
        """[(pulsar index, flag or None)]: the white-noise groups, the columns of theta's wn_efac / wn_log10_equad (_wn_hyper)"""
        return _wn_hyper.wn_groups(self.P, self._wn)

    @property
    def ecorr_groups(self):
        """[(pulsar index, flag or None)]: the ECORR groups, the columns of theta's wn_log10_ecorr (_wn_hyper)"""
        return _wn_hyper.ecorr_groups(self.P, self._ec)

    def _flag_array(self, a, flagid):
        return np.array([f[flagid] for f in self.psrs[a].toas.table["flags"].data])

    # ---------------------------------------------------------------- prepare -------------------
    def prepare(self):
        dev = dv.require_gpu()
        self._ws = None  # tables of a previous prepare() point at replaced buffers
        self._hy = None  # and the hyper path's tables describe the previous configuration
        self._wnh = None  # and so do the group tables of the per-realisation white noise
        self._chrom_t = None  # and the tables of the chromatic process
        self._cproc_t = None  # and those of the common processes
        self._td_prepared = False  # and so do the dense factors of TD mode
        self._gw_grid_ready = False
        s = dv.stream_ptr()
        P, N = self.P, self.n_toa
        self.d_psr_of = dv.i32(np.repeat(np.arange(P), self.counts))
        self.d_idx_in = dv.i32(np.concatenate([np.arange(c) for c in self.counts]))
        self.d_toa_s = dv.f64(np.concatenate([m.astype(float) * 86400 for m in self.mjd]))
        self.plan = _lib.EnginePlan()
        pl = self.plan
        pl.n_toa, pl.n_psr = N, P
        pl.idx_in_psr = self.d_idx_in.data_ptr()

        # ---- red noise: Ft [K, N] over the concatenated TOAs and amp = sqrt(prior) [P, K]
        pl.rn_k = 0
        if self._rn is not None:
            nm = self._rn["components"]
            K = 2 * nm
            self.K = K
            self.d_Ft = dv.zeros((K, N))
            amp = np.zeros((P, K))
            self.rn_freqs = []
            for a in range(P):
                lA, g = self._rn["A"][a], self._rn["g"][a]
                toas = self.tdb_s[a]
                Tspan = toas.max() - toas.min()
                f = 1.0 * np.arange(1, nm + 1) / Tspan
                self.rn_freqs.append(f)
                if lA is None or g is None:
                    continue
                freqs = np.repeat(f, 2)
                fyr = 1 / YEAR_IN_SEC
                prior = (10 ** lA) ** 2 * (freqs / fyr) ** (-g) / (12 * np.pi ** 2 * Tspan) * YEAR_IN_SEC ** 3
                amp[a] = np.sqrt(prior)
                t_d, f_d = dv.f64(toas), dv.f64(f)
                lib_conv = self._rn["libstempo"]
                t_ref = float(toas[0]) if lib_conv else 0.0
                _lib.call("pta_rn_basis", dv.ptr(t_d), len(toas), ctypes.c_double(t_ref), dv.ptr(f_d), None, nm,
                          1 if lib_conv else 0, ctypes.c_void_p(self.d_Ft.data_ptr() + 8 * int(self.off[a])), N, s)
            torch.cuda.current_stream().synchronize()  # t_d/f_d temporaries die with the loop
            self.rn_amp = amp
            self.d_amp = dv.f64(amp)
            pl.rn_k, pl.Ft, pl.ldf = K, self.d_Ft.data_ptr(), N

        # ---- EFAC / EQUAD vectors
        pl.wn_a = pl.wn_b = pl.wn_c = None
        if self._wn is not None:
            c = self._wn
            wa, wb = np.zeros(N), np.zeros(N)
            self.efacvec, self.equadvec = [], []
            for a in range(P):
                n = self.counts[a]
                efac = self._pick(c["efac"], a)
                l10 = self._pick(c["log10_equad"], a)
                flags = self._pick_flags(c["flags"], a)
                equad = 10 ** np.asarray(l10, dtype=float) if l10 is not None else 0.0
                if flags is None:
                    if not np.isscalar(efac) or np.ndim(equad) != 0:
                        raise ValueError("ERROR: If flags is None, efac and equad must be a scalar")
                    ev, qv = np.ones(n) * efac, np.ones(n) * float(equad)
                else:
                    ev, qv = np.zeros(n), np.zeros(n)
                    if not (len(efac) == len(flags) and len(equad) == len(flags)):
                        raise ValueError("ERROR: flags must be same length as efac and log10_equad")
                    tf = self._flag_array(a, c["flagid"])
                    for ct, flag in enumerate(flags):
                        ev[flag == tf] = efac[ct]
                        qv[flag == tf] = equad[ct]
                self.efacvec.append(ev)
                self.equadvec.append(qv)
                sl = slice(self.off[a], self.off[a + 1])
                wa[sl] = ev * self.sigma_s[a]
                wb[sl] = qv if c["tnequad"] else ev * qv
            self.d_wn_a, self.d_wn_b, self.d_wn_c = dv.f64(wa), dv.f64(wb), dv.f64(np.hypot(wa, wb))
            pl.wn_a, pl.wn_b, pl.tnequad = self.d_wn_a.data_ptr(), self.d_wn_b.data_ptr(), int(c["tnequad"])

        # ---- ECORR epoch maps
        pl.epoch_of = pl.ecorr_toa = None
        if self._ec is not None:
            c = self._ec
            ep_all, ec_all = np.zeros(N, dtype=np.int32), np.zeros(N)
            self.epoch_of, self.epoch_first, self.ecorrvec = [], [], []
            for a in range(P):
                l10 = self._pick(c["log10_ecorr"], a)
                flags = self._pick_flags(c["flags"], a)
                epoch_of, first = wn.epoch_map(self.mjd[a], c["coarsegrain"])
                ne = len(first)
                if l10 is None:
                    vec = np.zeros(ne)
                elif flags is None:
                    if not np.isscalar(l10):
                        raise ValueError("ERROR: If flags is None, jitter must be a scalar")
                    vec = np.ones(ne) * 10 ** l10
                else:
                    ecorr = 10 ** np.asarray(l10, dtype=float)
                    if len(ecorr) != len(flags):
                        raise ValueError("ERROR: flags must be same length as jitter")
                    aveflags = self._flag_array(a, c["flagid"])[first]
                    vec = np.zeros(ne)
                    for ct, flag in enumerate(flags):
                        vec[flag == aveflags] = ecorr[ct]
                self.epoch_of.append(epoch_of)
                self.epoch_first.append(np.asarray(first))
                self.ecorrvec.append(vec)
                sl = slice(self.off[a], self.off[a + 1])
                ep_all[sl] = epoch_of
                ec_all[sl] = vec[epoch_of]
            self.d_epoch_of, self.d_ecorr_toa = dv.i32(ep_all), dv.f64(ec_all)
            pl.epoch_of, pl.ecorr_toa = self.d_epoch_of.data_ptr(), self.d_ecorr_toa.data_ptr()

        # ---- workgroup tiles: <= ENGINE_TILE consecutive TOAs of ONE pulsar, plus the ECORR pair range they touch
        T = _lib.ENGINE_TILE
        t_psr, t_start, t_count, t_ep0, t_epn = [], [], [], [], []
        for a in range(P):
            for s0 in range(0, int(self.counts[a]), T):
                cnt = min(T, int(self.counts[a]) - s0)
                t_psr.append(a); t_start.append(int(self.off[a]) + s0); t_count.append(cnt)
                if self._ec is not None:
                    e = self.epoch_of[a][s0:s0 + cnt]
                    p0, p1 = int(e.min()) >> 1, int(e.max()) >> 1
                    t_ep0.append(p0); t_epn.append(p1 - p0 + 1 if p1 - p0 + 1 <= _lib.ENGINE_EPMAX else 0)
                else:
                    t_ep0.append(0); t_epn.append(0)
        self.d_tiles = [dv.i32(x) for x in (t_psr, t_start, t_count, t_ep0, t_epn)]
        pl.n_tiles = len(t_psr)
        pl.tile_psr, pl.tile_start, pl.tile_count, pl.tile_ep0, pl.tile_epn = [x.data_ptr() for x in self.d_tiles]

        # ---- GWB: grid, ORF, Cholesky, spectrum, twiddles, brackets
        pl.gw_npts = 0
        if self._gw is not None:
            c = self._gw
            grid = rn.gwb_time_grid(self.psrs_ideal_view(), c["npts"], c["howml"])
            self.grid = grid
            npts, Nf = grid["npts"], grid["Nf"]
            ORF = rn.gwb_orf_device(self.psrs, c["no_correlations"], c["clm"], c["lmax"])
            self.ORF = ORF.clone()
            self.d_M = rn.cholesky_device(ORF)
            # the basis ORFs of a configuration that can carry a clm per realisation (theta's gwb_clm): pta_gwb_orf_factor's operand
            self.d_orf_basis = None
            if _hyper.n_lm(c) is not None:
                self.d_orf_basis = anis.correlated_basis_device(rn.pulsar_locations(self.psrs), int(c["lmax"]))
            self.C = rn.gwb_spectrum(grid["f"], grid["dur"], c["howml"], c["A"], c["g"], c["turnover"], c["f0"], c["beta"],
                                     c["power"], c["userSpec"])
            self.ldt = rn.pad16(npts)
            self.d_T = dv.empty((2 * (Nf - 2), self.ldt))
            sqrtC = dv.f64(self.C ** 0.5)
            _lib.call("pta_gwb_twiddle", dv.ptr(sqrtC), Nf, npts, 10, ctypes.c_double(1.0 / grid["dt"]), dv.ptr(self.d_T), self.ldt, s)
            # throughput-mode layout of the same twiddles: half window, slab-major, plus the per-bin rotation
            nrot = ctypes.c_int64(0)
            nsym = _lib.lib.pta_gwb_twiddle_sym_size(Nf, npts, self.idft_variant, ctypes.byref(nrot))
            self._idft_variant_built = self.idft_variant
            self.d_Tsym, self.d_rot = dv.empty((nsym,)), dv.empty((nrot.value,))
            _lib.call("pta_gwb_twiddle_sym", dv.ptr(sqrtC), Nf, npts, 10, ctypes.c_double(1.0 / grid["dt"]), dv.ptr(self.d_Tsym),
                      dv.ptr(self.d_rot), self.idft_variant, s)
            # chirp-z tables (default frequency -> time transform whenever one 4096-point convolution covers the window)
            self.use_czt = bool(_lib.lib.pta_gwb_czt_fits(Nf, npts, 10)) and self.gwb_transform != "gemm"
            self.d_czt = None
            if self.use_czt:
                self.d_czt = [dv.empty((2 * 4096,)), dv.empty((2 * 4096,)), dv.empty((2 * 4096,)), dv.empty((2 * npts,))]
                _lib.call("pta_gwb_czt_setup", dv.ptr(sqrtC), Nf, npts, 10, ctypes.c_double(1.0 / grid["dt"]),
                          *[dv.ptr(x) for x in self.d_czt], s)
            self.d_ut = dv.f64(grid["ut"])
            self.d_jlo = dv.empty((N,), dtype=torch.int32)
            _lib.call("pta_gwb_bracket", dv.ptr(self.d_ut), npts, dv.ptr(self.d_toa_s), N, dv.ptr(self.d_jlo), s)
            torch.cuda.current_stream().synchronize()
            self.d_gw_w = dv.empty((N,))
            _lib.call("pta_gwb_weights", dv.ptr(self.d_ut), npts, dv.ptr(self.d_toa_s), dv.ptr(self.d_jlo), N, dv.ptr(self.d_gw_w), s)
            torch.cuda.current_stream().synchronize()
            pl.gw_npts, pl.gw_jlo, pl.gw_w = npts, self.d_jlo.data_ptr(), self.d_gw_w.data_ptr()

        # ---- deterministic signals (CGW), summed once
        pl.det = None
        extra = getattr(self, "_delays", None)
        if self._det or extra is not None:
            self.d_det = dv.zeros((N,)) if extra is None else dv.f64(extra)
            mjd_all = dv.f64(np.concatenate(self.mjd)) if self._det else None     # one upload; the kernel takes host scalars per call
            for kw in self._det or []:
                for a in range(P):
                    ra, dec = ra_dec(self.psrs[a])
                    par, _, _, _ = det.cgw_parameters(np.pi / 2 - dec, ra, **{k: v for k, v in kw.items() if k != "signal_name"})
                    par = np.ascontiguousarray(par)          # copied into the kernel argument at launch: no lifetime issue
                    o = int(self.off[a])
                    _lib.call("pta_cgw", ctypes.c_void_p(mjd_all.data_ptr() + 8 * o), len(self.mjd[a]), dv.hptr(par),
                              ctypes.c_void_p(self.d_det.data_ptr() + 8 * o), 1, s)
            if self._det:
                torch.cuda.current_stream().synchronize()      # once, not once per pulsar per source
            pl.det = self.d_det.data_ptr()
        if self._chrom is not None:
            self._prepare_chrom()
        if self._cproc:
            self._prepare_cproc()
        self._prepared = True
        # set-up time is where one-off driver costs belong: with measurement noise configured the dense path can follow, and the
        # factorisation's internal streams (hardware queues, ~10 ms each on this stack: profiles/r05_prepare_td_first_call.txt) are
        # created now instead of inside the first prepare_td() (td_warmup = False leaves them to be created on demand)
        if self._wn is not None and getattr(self, "td_warmup", True):
            _lib.call("pta_potrf_warmup", 2)
        return self

    def _chrom_host_tables(self):
        """the host half of the chromatic tables, NumPy alone: the row weights w [n_toa] = (nu_ref / nu_i)^chi, per pulsar the
        frequencies k / Tspan [K_c / 2], Tspan [P], and the configured sqrt(prior) amp [P, K_c] (a row of zeros = no process)"""
        c = self._chrom
        P, nm = self.P, c["components"]
        w = np.concatenate([_chrom.weights(_chrom.toa_freqs(p), c["index"], c["ref"], name=f"pulsar {p.name}") for p in self.psrs])
        amp, freqs, tspan = np.zeros((P, 2 * nm)), [], np.zeros(P)
        for a in range(P):
            lA, g = c["A"][a], c["g"][a]
            toas = self.tdb_s[a]
            tspan[a] = toas.max() - toas.min()
            freqs.append(1.0 * np.arange(1, nm + 1) / tspan[a])
            if lA is not None and g is not None:
                amp[a] = np.sqrt(_chrom.prior_phi(freqs[a], tspan[a], lA, g))
        return dict(K=2 * nm, w=w, amp_host=amp, freqs=freqs, tspan_host=tspan)

    def _prepare_chrom(self):
        """the tables of the chromatic process (self._chrom_t), buffers of their own beside everything prepare() built: the weighted design
        matrix Ft [K_c, n_toa] (pta_rn_basis, its rows then scaled by the host's weights - no device pow), the configured amplitudes amp
        [P, K_c], and frequencies [P, K_c / 2] and Tspan [P] of the theta path"""
        t = self._chrom_host_tables()
        c = self._chrom
        N, nm = self.n_toa, c["components"]
        s = dv.stream_ptr()
        Ft = dv.zeros((t["K"], N))
        keep = []
        for a in range(self.P):
            if c["A"][a] is None or c["g"][a] is None:
                continue
            t_d, f_d = dv.f64(self.tdb_s[a]), dv.f64(t["freqs"][a])
            keep += [t_d, f_d]
            _lib.call("pta_rn_basis", dv.ptr(t_d), len(self.tdb_s[a]), ctypes.c_double(0.0), dv.ptr(f_d), None, nm, 0,
                      ctypes.c_void_p(Ft.data_ptr() + 8 * int(self.off[a])), N, s)
        Ft *= dv.f64(t["w"]).unsqueeze(0)
        torch.cuda.current_stream().synchronize()  # the temporaries die with the call
        t.update(Ft=Ft, amp=dv.f64(t["amp_host"]), f=dv.f64(np.stack(t["freqs"])), tspan=dv.f64(t["tspan_host"]))
        self._chrom_t = t

    def _chrom_low_rank_host(self):
        """(F [P][N_a, K_c], phi [P][K_c]): the weighted chromatic basis w_i times sin / cos of 2 pi f t as prepare() puts it on the
        device, and the configured prior - the columns the fixed-noise statistics add to the low-rank part of C_a.  NumPy alone."""
        t = self._chrom_t if self._chrom_t is not None else self._chrom_host_tables()
        F_all = []
        for a in range(self.P):
            tdb, f = self.tdb_s[a], t["freqs"][a]
            arg = 2 * np.pi * tdb[:, None] * f[None, :]
            F = np.empty((len(tdb), 2 * len(f)))
            F[:, 0::2], F[:, 1::2] = np.sin(arg), np.cos(arg)
            F_all.append(t["w"][self.off[a]:self.off[a + 1], None] * F)
        return F_all, [t["amp_host"][a] ** 2 for a in range(self.P)]

    def psrs_ideal_view(self):
        """objects exposing first_MJD/last_MJD of the IDEAL TOAs for the GWB grid (red_noise.py:182-183)."""
        class _V:
            pass
        out = []
        for m in self.mjd:
            v = _V()
            v.toas = _V()
            v.toas.first_MJD = _V()
            v.toas.last_MJD = _V()
            v.toas.first_MJD.value = float(m.min())
            v.toas.last_MJD.value = float(m.max())
            out.append(v)
        return out

    def _pick(self, val, a):
        """per-pulsar entry of a scalar / list-of-P parameter."""
        if val is None or np.isscalar(val):
            return val
        if len(val) != self.P:
            raise ValueError(f"expected a scalar or one entry per pulsar ({self.P}), got {len(val)}")
        return val[a]

    def _pick_flags(self, flags, a):
        if flags is None:
            return None
        if len(flags) != self.P:
            raise ValueError("flags must be a per-pulsar list of flag lists")
        return flags[a]

    # ---------------------------------------------------------------- throughput mode -----------
    def workspace(self, R):
        """device buffers for a batch of R realisations (reused across generate() calls) and the pta_engine_tables that
        point at them."""
        ws = getattr(self, "_ws", None)
        if ws is None or ws["R"] < R:
            ws = {"R": R}
            tb = _lib.EngineTables()
            if self.plan.rn_k:
                ws["coef"] = dv.empty((R, self.P, self.K))
                tb.rn_amp, tb.ws_coef = self.d_amp.data_ptr(), ws["coef"].data_ptr()
            if self.plan.gw_npts:
                ws["G0"] = dv.empty((R, self.P, self.plan.gw_npts))
                ws["G"] = dv.empty((R, self.P, self.plan.gw_npts))
                tb.Mchol, tb.ws_G0, tb.ws_G = self.d_M.data_ptr(), ws["G0"].data_ptr(), ws["G"].data_ptr()
                tb.gw_nf, tb.gw_i0 = self.grid["Nf"], 10
                if getattr(self, "d_czt", None) is not None:
                    tb.czt_pre, tb.czt_FB, tb.czt_tw, tb.czt_post = (x.data_ptr() for x in self.d_czt)
                tb.Tsym, tb.rot = self.d_Tsym.data_ptr(), self.d_rot.data_ptr()
                tb.idft_variant = self._idft_variant_built
            ws["tables"] = tb
            self._ws = ws
        ws["tables"].czt_variant, ws["tables"].mix_variant = int(self.czt_variant), int(self.mix_variant)
        if self.plan.gw_npts:
            if self.use_czt and getattr(self, "d_czt", None) is None:
                raise ValueError("use_czt was switched on after prepare(): the chirp-z tables were not built")
            ws["tables"].use_czt = 1 if self.use_czt else 0
        self.plan.rng_fast, self.plan.synth_variant = int(self.rng_fast), int(self.synth_variant)
        return ws

    def max_batch(self, hyper=False, cw=False, clm=False):
        """realisations per launch sequence: the launch-grid limit of the mix / fused kernels (65536) and the workspace byte
        budget (coef + G0 + G per realisation: 0.68 MB at 68 pulsars, so 8 GiB hold 12 600 realisations; with per-realisation
        theta (hyper=True) also the GWB spectrum-scale row, 8 Nf bytes; with CW theta (cw=True) also the CW source row and the
        [P, 16] scalar table of pta_engine_cw_params; cw = S, an integer: a catalogue of S sources per realisation, S source rows
        and the [P, S, 16] table of pta_engine_cw_catalog_params, whose one-launch index range R P S < 2^31 also bounds the batch;
        with gwb_clm in theta (clm=True) also the realisation's ORF factor [P, P] and its info word, and pta_gwb_mix_batched's one
        workgroup row per realisation bounds the batch at 65535)."""
        per_real = 8 * self.P * ((self.K if self.plan.rn_k else 0) + 2 * self.plan.gw_npts)
        if hyper and self.plan.gw_npts:
            per_real += 8 * self.grid["Nf"]
        cap = 65536
        if clm:
            per_real += 8 * self.P * self.P + 4
            cap = 65535
        if cw:
            S = 1 if cw is True else int(cw)
            if S < 1:
                raise ValueError(f"max_batch: cw must be True, False or a source count >= 1, got {cw!r}")
            per_real += 8 * (self.P * S * _lib.CW_ENGINE_NPAR + _cw.N_SRC * S + self.P)
            cap = min(cap, ((1 << 31) - 1) // (self.P * S))
        return int(max(1 if cap < 16 else 16, min(cap, self.workspace_bytes // max(per_real, 1))))

    def generate(self, R, r0=0, out=None, theta=None):
        """out[R, n_toa] (device tensor, seconds): realisations r0 .. r0+R-1, every deviate drawn on chip: one call of
        pta_engine_generate (coefficients -> GWB transform -> mix -> fused synthesis, all queued on the current stream).

        theta: per-realisation GWB / red-noise parameters of realisations r0 .. r0+R-1, a dict with any subset of
        gwb_log10_A [R], gwb_gamma [R], rn_log10_A [R, P], rn_gamma [R, P] (NumPy arrays or tensors; pta_replicator_amd._hyper).
        Keys not given keep their configured values; NaN in rn_log10_A = that pulsar as configured.  On an engine configured with
        set_gwb(userSpec=U [M, 2]) theta may hold gwb_log10_hc [R, M] instead of the two GWB keys: row r replaces log10(U[:, 1]) for
        realisation r0 + r (column j = row j of U as given), with the reference's userSpec semantics (log10 hc linear in log10 f
        between the nodes, constant outside them); pta_gwb_spectrum_scale_user then fills the scale row.  With set_cw(), theta may also
        hold one CW source per realisation (cw_* keys, pta_replicator_amd._cw), added by pta_engine_cw_add after the batch, or a
        catalogue of S sources per realisation (the same keys with shape [R, S], optional cw_count [R]), summed over the sources and
        added once by pta_engine_cw_catalog_add.  With set_bwm(), theta may hold one burst with memory per realisation (the five bwm_*
        keys, pta_replicator_amd._bwm), added by pta_engine_bwm_add after the CW term.  With set_burst() / set_transients(), theta may hold a
        burst of sine-Gaussian wavelets and noise transients per realisation (the burst_* and nt_* keys, pta_replicator_amd._burst),
        added after the BWM term by pta_engine_burst_add and then pta_engine_transient_add.  With set_chromatic_events(), theta may hold
        chromatic events per realisation (the ce_* keys, pta_replicator_amd._chrom_event), added after the noise transients by
        pta_engine_chrom_event_add.  On an engine configured with set_gwb(lmax=L >= 1)
        (correlated, gwb_mode "fourier") theta may hold gwb_clm [R, (L+1)^2]: row r replaces the configured clm for realisation r0 + r
        (column k = l^2 + m + l, correlated_basis' order), with the reference's semantics, ORF_r = 2 sum_k clm_r[k] basis[k],
        M_r = chol(ORF_r), G_r = M_r G0_r: pta_gwb_orf_factor fills the factors ahead of each batch and pta_gwb_mix_batched mixes with
        them.  A row whose ORF is not positive definite raises numpy.linalg.LinAlgError after the call's last batch (its realisation
        is all NaN).  The key combines freely with every other one.  On an engine configured with set_white_noise / set_jitter
        (wn_mode "reference") theta may hold the white-noise parameters of every group: wn_efac [R, G_wn], wn_log10_equad [R, G_wn],
        wn_log10_ecorr [R, G_ec] (pta_replicator_amd._wn_hyper; the columns are engine.wn_groups / engine.ecorr_groups, (pulsar, flag)
        pairs, pulsar-major).  Each entry replaces the configured value of its group for realisation r0 + r, NaN = as configured; a key
        given alone leaves the other parameters as configured, tnequad keeps its configured meaning, and a TOA (or epoch) whose flag is
        in no listed group keeps amplitude 0.  The fused launch then runs without the terms that have a key and pta_engine_wn_add
        redraws the same deviates (same stream, same counter: dump_draws is unchanged) with the realisation's own amplitudes, ahead
        of the CW / BWM terms.  Fixed-noise statistics evaluated on such realisations (generate_os and the other generate_* with these
        keys in the generation theta) weight with the configured white noise, as they do for red-noise keys; as a statistic's noise
        model (optimal_statistic(theta=), matched=True, likelihood grids), in TD mode and in wn_mode "single" the keys are refused.  On an engine
        configured with set_chromatic_noise theta may hold chrom_log10_A, chrom_gamma [R, P] (pta_replicator_amd._chrom), with the rules of
        the red-noise keys; the chromatic term is added last, after the CW / BWM terms."""
        hyper, cw = self._theta_parts(theta, R)
        return self._generate(R, r0, out, hyper, cw)

    def _generate(self, R, r0, out, hyper, cw, mask_unconfigured=True, raise_orf=True):
        """generate() for theta resolved by _theta_parts, one launch sequence per batch: pta_engine_generate (hyper None) or
        pta_engine_generate_hyper (red-noise coefficients with sqrt(prior) per realisation -> spectrum scale -> scaled GWB transform ->
        mix -> the unchanged fused synthesis); gwb_mode "grid" queues the same stages one by one, the grid factor's product as the GWB
        transform.  With gwb_clm in hyper pta_gwb_orf_factor is queued ahead of each batch and the mix reads its factors; info of the whole
        call [R] is read once after the last batch and a non-zero entry raises LinAlgError (raise_orf=False: left in self._orf_info,
        the label of generate_sampled).  With white-noise keys in cw the fused launch runs on a private plan copy without the terms that have a
        key, and pta_engine_wn_params + pta_engine_wn_add follow it batch by batch (_wn_add).  Then the CW / BWM terms of cw.
        mask_unconfigured: as in _theta_device."""
        if not self._prepared:
            self.prepare()
        dev = None if hyper is None else self._theta_device(hyper, R, mask_unconfigured)
        if out is None:
            out = dv.empty((R, self.n_toa))
        clm = None if dev is None else dev[_hyper.CLM_KEY]
        step = self.max_batch(hyper=hyper is not None, cw=_cw.n_sources(cw), clm=clm is not None)
        ws = self.workspace(min(R, step))
        hy = None if dev is None else self._hyper_tables()
        info = None
        if clm is not None:
            if "mchol" not in ws or ws["mchol"].shape[0] < ws["R"]:
                ws["mchol"] = dv.empty((ws["R"], self.P, self.P))
            info = self._orf_info = dv.zeros((R,), dtype=torch.int32)
        gw_theta = dev is not None and dev["gwb_log10_A"] is not None
        spec = None if dev is None else dev[_hyper.SPEC_KEY]
        if (gw_theta or spec is not None) and ("scale" not in ws or ws["scale"].shape[0] < ws["R"]):
            ws["scale"] = dv.empty((ws["R"], self.grid["Nf"]))
        grid_mode = self.gwb_mode == "grid" and self.plan.gw_npts
        if grid_mode:
            self._prepare_gw_grid_factor()
            self.tdgw_plan.rng_fast = int(self.rng_fast)
            self.tdgw_plan.z, self.tdgw_plan.ld_z, self.tdgw_plan.blk_zoff = None, 0, None   # (generate_td may have pointed it at a deviate buffer)
        s = dv.stream_ptr()
        P = self.P
        at = dv.row_ptr
        plan = self._plan_for_mode()
        wdev = None
        if _wn_hyper.has_keys(cw):   # the terms that have a key leave the fused launch: a private plan copy, the shared one is never mutated
            wdev = self._wn_theta_device(cw, R)
            plan = _lib.EnginePlan.from_buffer_copy(self.plan)
            if wdev["wn"]:
                plan.wn_a = plan.wn_b = None
            if wdev["ecorr"]:
                plan.ecorr_toa = plan.epoch_of = None
        for lo in range(0, R, step):
            n = min(step, R - lo)
            optr = at(out, lo)
            h = None
            if dev is not None:
                h = _lib.EngineHyper()
                if self.plan.rn_k:
                    h.rn_f, h.rn_tspan = hy["rn_f"].data_ptr(), hy["rn_tspan"].data_ptr()
                    h.rn_log10_A, h.rn_gamma = at(dev["rn_log10_A"], lo), at(dev["rn_gamma"], lo)
                if gw_theta:
                    h.ld_gw_scale, h.ws_scale = self.grid["Nf"], ws["scale"].data_ptr()
                    h.gw_log10_A, h.gw_gamma = at(dev["gwb_log10_A"], lo), at(dev["gwb_gamma"], lo)
                    h.gw_f, h.gw_hcf0 = hy["gw_f"].data_ptr(), hy["gw_hcf0"].data_ptr()
                    c = self._gw
                    h.gw_turnover, h.gw_f0, h.gw_beta, h.gw_power = int(bool(c["turnover"])), float(c["f0"]), float(c["beta"]), float(c["power"])
                if spec is not None:   # the scale row from the realisation's own spectrum, queued ahead of the launch sequence
                    Nf, M = self.grid["Nf"], spec.shape[1]
                    _lib.call("pta_gwb_spectrum_scale_user", dv.ptr(hy["spec_seg"]), dv.ptr(hy["spec_dx"]), dv.ptr(hy["spec_dxp"]),
                              dv.ptr(hy["gw_hcf0"]), Nf, M, n, at(spec, lo), M, dv.ptr(ws["scale"]), Nf, s)
                    h.gw_scale, h.ld_gw_scale = ws["scale"].data_ptr(), Nf
                if clm is not None:    # the ORF factor of every realisation of the batch, queued ahead of the launch sequence
                    _lib.call("pta_gwb_orf_factor", dv.ptr(self.d_orf_basis), clm.shape[1], P, at(clm, lo), clm.stride(0), n, dv.ptr(ws["mchol"]),
                              ctypes.c_void_p(info.data_ptr() + 4 * lo), s)
                    h.gw_mchol, h.ld_gw_mchol = ws["mchol"].data_ptr(), P * P
            if not grid_mode:
                args = (self.seed, r0 + lo, n, optr, out.stride(0), s)
                if h is None:
                    _lib.call("pta_engine_generate", ctypes.byref(plan), ctypes.byref(ws["tables"]), *args)
                else:
                    _lib.call("pta_engine_generate_hyper", ctypes.byref(plan), ctypes.byref(ws["tables"]), ctypes.byref(h), *args)
                if wdev is not None:
                    self._wn_add(wdev, lo, n, r0 + lo, optr, out.stride(0))
                continue
            pl = _lib.EnginePlan.from_buffer_copy(plan)    # grid mode: RN theta only (check_config)
            if pl.rn_k:
                if h is not None and h.rn_log10_A:
                    _lib.call("pta_engine_rn_coef_hyper", self.seed, r0 + lo, n, P, self.K, h.rn_f, h.rn_tspan, h.rn_log10_A, h.rn_gamma,
                              dv.ptr(self.d_amp), dv.ptr(ws["coef"]), int(self.rng_fast), s)
                else:
                    _lib.call("pta_engine_rn_coef", self.seed, r0 + lo, n, P, self.K, dv.ptr(self.d_amp), dv.ptr(ws["coef"]), int(self.rng_fast), s)
                pl.rn_coef = ws["coef"].data_ptr()
            _lib.call("pta_td_trmm_rng", ctypes.byref(self.tdgw_plan), self.seed, r0 + lo, n * P, dv.ptr(ws["G0"]), pl.gw_npts, s)
            _lib.call("pta_gwb_mix", dv.ptr(self.d_M), P, dv.ptr(ws["G0"]), n, pl.gw_npts, pl.gw_npts, dv.ptr(ws["G"]), int(self.mix_variant), s)
            pl.gw_G = ws["G"].data_ptr()
            _lib.call("pta_engine_synth", ctypes.byref(pl), self.seed, r0 + lo, n, optr, out.stride(0), s)
            if wdev is not None:
                self._wn_add(wdev, lo, n, r0 + lo, optr, out.stride(0))
        # per-kernel callers (bench.py, replay) read the workspace pointers from the plan
        if self.plan.rn_k:
            self.plan.rn_coef = ws["coef"].data_ptr()
        if self.plan.gw_npts:
            self.plan.gw_G = ws["G"].data_ptr()
        if dev is not None:
            self._keep["theta"] = dev   # the launches above read these buffers asynchronously
        if wdev is not None:
            self._keep["wn"] = wdev
        if info is not None and raise_orf:
            bad = torch.nonzero(info).flatten()
            if bad.numel():
                raise np.linalg.LinAlgError(f"Matrix is not positive definite (gwb_clm of realisation {r0 + int(bad[0])}: its ORF)")
        if cw:
            self._det_apply(cw, R, out)
        if self._chrom is not None:   # last, so that a row is the row of the engine without the process plus the term: one add
            self._chrom_apply(cw, R, r0, out)
        if self._cproc:   # after it, by the same rule: the engine without the processes plus generate_per_signal()["common"], one add
            self._cproc_apply(cw, R, r0, out)
        return out

    def _theta_device(self, th, R, mask_unconfigured=True):
        """validated theta -> contiguous float64 device tensors, keys not given filled with the configured values:
        {gwb_log10_A, gwb_gamma: [R] or None, rn_log10_A, rn_gamma: [R, P] or None, gwb_log10_hc: [R, M] or None, its columns in
        ascending node frequency, gwb_clm: [R, n_lm] or None}.  Pulsars without red noise get NaN amplitudes (mask_unconfigured=False: theta of sample_theta, which
        has them already)."""
        dev = dict.fromkeys(_hyper.ALL_KEYS)
        if _hyper.SPEC_KEY in th:
            dev[_hyper.SPEC_KEY] = self._spec_theta_device(th)
        if _hyper.CLM_KEY in th:
            dev[_hyper.CLM_KEY] = dv.as_f64(th[_hyper.CLM_KEY])
        if any(k in th for k in _hyper.GWB_KEYS):
            for k, conf in (("gwb_log10_A", self._gw["A"]), ("gwb_gamma", self._gw["g"])):
                dev[k] = dv.as_f64(th[k]) if k in th else torch.full((R,), float(conf), dtype=torch.float64, device=dv.require_gpu())
        if any(k in th for k in _hyper.RN_KEYS) and self.plan.rn_k:
            self._rn_theta_device(th, R, dev, mask_unconfigured)
        return dev

    def _spec_theta_device(self, th):
        """theta's gwb_log10_hc -> [R, M] on the device, its columns in ascending node frequency"""
        y = dv.as_f64(th[_hyper.SPEC_KEY])
        order = self._hyper_tables()["spec_order"]
        return y if order is None else y.index_select(1, order).contiguous()

    def _rn_theta_device(self, th, R, dev, mask_unconfigured=True):
        """dev's rn_log10_A and rn_gamma [R, P] from validated theta, a key not given filled with the configured values; pulsars
        configured without red noise get NaN amplitudes (mask_unconfigured)"""
        for k, c in zip(_hyper.RN_KEYS, _hyper.configured_rn(self._rn)):
            dev[k] = dv.as_f64(th[k]) if k in th else dv.f64(np.ascontiguousarray(np.broadcast_to(c, (R, self.P))))
        none = self._hyper_tables()["rn_none"]
        if mask_unconfigured and len(none):   # configured without red noise: keeps none (amp_fixed row is zero)
            dev["rn_log10_A"] = dev["rn_log10_A"].clone()
            dev["rn_log10_A"][:, none] = float("nan")

    def _hyper_tables(self):
        """theta-independent device tables of the hyper path, built once per prepare(): GWB frequency grid and configured hcf,
        red-noise frequencies [P, K/2] and Tspan [P] (the values prepare() built the configured amplitudes from).  With a userSpec
        that can carry a per-realisation spectrum: per grid bin the segment, x - xp[segment] and the node spacing (_hyper.spec_tables)
        and the node order (None = the nodes were given sorted)."""
        if self._hy is not None:
            return self._hy
        hy = {}
        if self.plan.gw_npts:
            c = self._gw
            hy["gw_f"] = dv.f64(self.grid["f"])
            if c["userSpec"] is None:
                hy["gw_hcf0"] = dv.f64(rn.gwb_spectrum_hcf(self.grid["f"], c["A"], c["g"], c["turnover"], c["f0"], c["beta"], c["power"]))
            else:
                try:
                    order, xp = _hyper.spec_nodes(c["userSpec"])
                except ValueError:      # a userSpec no spectrum key can use (refused by _hyper.check_config when one is given)
                    order = None
                else:
                    seg, dx, dxp = _hyper.spec_tables(self.grid["f"], xp)
                    hy["spec_seg"], hy["spec_dx"], hy["spec_dxp"] = dv.i32(seg), dv.f64(dx), dv.f64(dxp)
                    hy["gw_hcf0"] = dv.f64(rn.gwb_spectrum_hcf(self.grid["f"], c["A"], c["g"], userSpec=np.asarray(c["userSpec"], dtype=np.float64)))
                    order = None if np.array_equal(order, np.arange(len(order))) else dv.i64(order)
                hy["spec_order"] = order
        if self.plan.rn_k:
            hy["rn_f"] = dv.f64(np.stack(self.rn_freqs))
            hy["rn_tspan"] = dv.f64(np.array([t.max() - t.min() for t in self.tdb_s]))
            hy["rn_none"] = dv.i64(np.flatnonzero(np.isnan(_hyper.configured_rn(self._rn)[0])))
        self._hy = hy
        return hy

    def generate_sampled(self, R, r0=0, out=None):
        """(out[R, n_toa], theta): realisations r0 .. r0+R-1 with theta drawn on chip from the set_hyper_prior() boxes
        (pta_hyper_uniform: uniform u2 of stream (7, 0), pair = parameter column, so theta of realisation r is a pure function of
        (seed, r) like its residuals).  theta: {key: device tensor} of the sampled keys, gwb_* [R], rn_* [R, P] (NaN for pulsars
        without red noise) - the labels of the realisations.  A sampled spectrum comes back as gwb_log10_hc [R, M], node j drawn from
        stream (7, 1), pair j (pta_hyper_uniform_field), so the columns of stream (7, 0) and their labels do not move.  A sampled sky
        comes back as gwb_clm [R, n_lm] (columns l >= 1 from stream (7, 2), pair = column; column 0 the configured c_00) with
        gwb_orf_info [R] int32: 0, or the 1-based pivot at which the row's ORF stopped being positive definite - such a realisation is
        all NaN and flagged, not raised.  Sampled white noise comes back as wn_efac, wn_log10_equad [R, G_wn] and wn_log10_ecorr
        [R, G_ec], group j drawn from stream (7, 3), (7, 4), (7, 5), pair j: no other label or residual moves.  With set_population()
        theta also holds population_theta(R, r0): gwb_log10_hc [R, F], the cw_* keys [R, S] with cw_count [R], and the labels pop_cell,
        pop_number [R, S] (streams (11, attempt) and (8, s)).  With set_burst_prior() / set_transient_prior() theta holds the burst_* keys
        (sky labels from stream (13, 0), wavelet w from stream (13, 1 + w)) and the nt_* keys (transient v from stream (14, v); nt_psr
        int32, the floor of a U(0, P) draw).  With set_chromatic_event_prior() theta holds the ce_* keys (slot e from stream (15, e); ce_psr
        and ce_kind int32)."""
        prior, cw_prior, bwm_prior = getattr(self, "_prior", None), getattr(self, "_cw_prior", None), getattr(self, "_bwm_prior", None)
        wn_prior, chrom_prior, cp_prior = getattr(self, "_wn_prior", None), getattr(self, "_chrom_prior", None), getattr(self, "_cproc_prior", None)
        burst_prior, nt_prior = getattr(self, "_burst_prior", None), getattr(self, "_nt_prior", None)
        if (prior is None and cw_prior is None and bwm_prior is None and wn_prior is None and chrom_prior is None and cp_prior is None
                and getattr(self, "_pop", None) is None and burst_prior is None and nt_prior is None and getattr(self, "_ce_prior", None) is None):
            raise ValueError("generate_sampled: no prior (set_hyper_prior / set_cw_prior / set_bwm_prior first)")
        if cp_prior is not None and not self._cproc:
            raise ValueError("generate_sampled: common-process boxes given but no common process is configured (add_common_process)")
        if chrom_prior is not None and self._chrom is None:
            raise ValueError("generate_sampled: chromatic boxes given but no chromatic process is configured (set_chromatic_noise)")
        if prior is not None:
            _hyper.check_config(prior.keys(), self._gw, self._rn, self.gwb_mode)
        if wn_prior is not None:
            _wn_hyper.check_config(wn_prior.keys(), self.P, self._wn, self._ec, self.wn_mode)
        if cw_prior is not None and self._cw is None:
            raise ValueError("generate_sampled: no per-realisation CW configured (set_cw)")
        if bwm_prior is not None and not self._bwm:
            raise ValueError("generate_sampled: no per-realisation burst with memory configured (set_bwm)")
        if burst_prior is not None and self._burst is None:
            raise ValueError("generate_sampled: no per-realisation wavelet burst configured (set_burst)")
        if nt_prior is not None and self._nt is None:
            raise ValueError("generate_sampled: no per-realisation noise transients configured (set_transients)")
        if not self._prepared:
            self.prepare()
        theta = self._sample_theta(R, r0, orf_info=False)
        hyper, cw = self._theta_parts(theta, R, check_values=False)
        out = self._generate(R, r0, out, hyper, cw, mask_unconfigured=False, raise_orf=False)
        if _hyper.CLM_KEY in theta:
            theta[_hyper.ORF_INFO_KEY] = self._orf_info
        return out, theta

    def _plan_for_mode(self):
        """the plan generate() launches with: the shared one, or - wn_mode "single" - a private copy whose white-noise operands are
        replaced by the combined amplitude vector (pta_engine_plan.wn_c)."""
        if self.wn_mode == "reference" or not self.plan.wn_a:
            return self.plan
        if self.wn_mode != "single":
            raise ValueError(f"wn_mode={self.wn_mode!r} must be 'reference' or 'single'")
        pl = _lib.EnginePlan.from_buffer_copy(self.plan)
        pl.wn_a = pl.wn_b = None
        pl.wn_c = self.d_wn_c.data_ptr()
        return pl

    def _require_reference_draws(self, what):
        """the replay entry points describe the reference's draws (two deviates per TOA, white_noise.py:105-109): in wn_mode "single"
        generate() draws something else, so they refuse instead of silently answering for another mode."""
        if self.wn_mode != "reference" and self._wn is not None:
            raise ValueError(f"{what}() describes the reference-order draws; wn_mode={self.wn_mode!r} realisations are not replayable "
                             "(use dump_draws_wn_single / generate_per_signal, or set wn_mode = 'reference')")

    def dump_draws_wn_single(self, r):
        """the ONE deviate per TOA realisation r uses in wn_mode "single": TOA idx of pulsar a takes branch (idx >> 4) & 1 of pair
        idx & ~16 of stream (WN, a) - one array per pulsar."""
        s = dv.stream_ptr()
        out = []
        for a in range(self.P):
            n = int(self.counts[a])
            z0, z1 = dv.empty((n,)), dv.empty((n,))
            _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_WN, a), n, 0, dv.ptr(z0), dv.ptr(z1), n, int(self.rng_fast), s)
            idx = np.arange(n)
            z0, z1 = z0.cpu().numpy(), z1.cpu().numpy()
            out.append(np.where((idx >> 4) & 1, z1[idx & ~16], z0[idx & ~16]))
        return out

    def generate_per_signal(self, R, r0=0, theta=None):
        """{'rn', 'gwb', 'wn', 'ecorr', 'det', 'total'}: the same realisations as generate(R, r0), one [R, n_toa] array per
        signal (the batched counterpart of the reference's per-signal ``added_signals_time`` entries).  Every deviate is a pure
        function of (seed, realisation, stream, index), so running the fused kernel once per signal with the other inputs
        switched off reproduces exactly the deviates of the combined pass.  theta: per-realisation parameters as in generate(); with
        CW keys the dict also has 'cw', the per-realisation CW term (pta_engine_cw_add writing its own buffer; for a catalogue the
        sum over its sources, pta_engine_cw_catalog_add); with BWM keys 'bwm', the per-realisation burst-with-memory term alone
        (pta_engine_bwm_add writing its own buffer); with burst_* keys 'burst' and with nt_* keys 'transient', the wavelet burst and the
        noise transients alone (pta_engine_burst_add / pta_engine_transient_add writing their own buffers); with ce_* keys 'chrom_event', the
        chromatic events alone (pta_engine_chrom_event_add writing its own buffer); with white-noise keys (wn_efac / wn_log10_equad, wn_log10_ecorr) 'wn' and 'ecorr' are the
        per-realisation terms (pta_engine_wn_add writing its own buffer); on an engine with a chromatic process
        (set_chromatic_noise) 'chrom', that term alone (pta_engine_chrom_add writing its own buffer)."""
        hyper, cw = self._theta_parts(theta, R)
        if not self._prepared:
            self.prepare()
        step = self.max_batch(hyper=theta is not None, cw=_cw.n_sources(cw), clm=hyper is not None and _hyper.CLM_KEY in hyper)
        if R > step:
            raise ValueError(f"generate_per_signal: at most {step} realisations per call (one workspace batch)")
        total = self._generate(R, r0, None, hyper, cw)       # also fills the workspace (coefficients, mixed GWB grid series)
        s = dv.stream_ptr()
        base = self._plan_for_mode()                         # wn_mode "single": the white-noise term is the one-deviate form, as in generate()
        keep = (self.plan.rn_k, self.plan.gw_npts, base.wn_a, base.wn_b, self.plan.ecorr_toa, self.plan.epoch_of, self.plan.det, base.wn_c)
        out = {"total": total}

        def one(name, **on):
            pl = _lib.EnginePlan.from_buffer_copy(self.plan)   # a private copy: the shared plan is never mutated
            pl.rn_k, pl.gw_npts, pl.wn_a, pl.wn_b, pl.ecorr_toa, pl.epoch_of, pl.det, pl.wn_c = (
                on.get("rn_k", 0), on.get("gw_npts", 0), on.get("wn_a"), on.get("wn_b"), on.get("ecorr_toa"),
                on.get("epoch_of"), on.get("det"), on.get("wn_c"))
            buf = dv.empty((R, self.n_toa))
            _lib.call("pta_engine_synth", ctypes.byref(pl), self.seed, r0, R, dv.ptr(buf), buf.stride(0), s)
            out[name] = buf
        if keep[0]:
            one("rn", rn_k=keep[0])
        if keep[1]:
            one("gwb", gw_npts=keep[1])
        wdev = self._wn_theta_device(cw, R) if _wn_hyper.has_keys(cw) else {"wn": False, "ecorr": False}

        def one_wn(name, **term):   # a term with a key in theta: the per-realisation term, pta_engine_wn_add writing its own buffer
            out[name] = dv.empty((R, self.n_toa))
            self._wn_add(wdev, 0, R, r0, dv.ptr(out[name]), out[name].stride(0), accumulate=False, **term)
        if wdev["wn"]:
            one_wn("wn", ecorr=False)
        elif keep[2] or keep[7]:
            one("wn", wn_a=keep[2], wn_b=keep[3], wn_c=keep[7])
        if wdev["ecorr"]:
            one_wn("ecorr", wn=False)
        elif keep[4]:
            one("ecorr", ecorr_toa=keep[4], epoch_of=keep[5])
        self._keep["wn"] = wdev
        if keep[6]:
            out["det"] = self.d_det.unsqueeze(0).expand(R, self.n_toa)
        if _cw.has_keys(cw):
            out["cw"] = self._cw_apply(cw, R, dv.empty((R, self.n_toa)), accumulate=False)
        if _bwm.has_keys(cw):
            out["bwm"] = self._bwm_apply(cw, R, dv.empty((R, self.n_toa)), accumulate=False)
        if _burst.has_keys(cw):      # 'burst': the wavelet burst alone (pta_engine_burst_add writing its own buffer)
            out["burst"] = self._burst_apply(cw, R, dv.empty((R, self.n_toa)), accumulate=False)
        if _burst.has_nt_keys(cw):   # 'transient': the noise transients alone (pta_engine_transient_add writing its own buffer)
            out["transient"] = self._nt_apply(cw, R, dv.empty((R, self.n_toa)), accumulate=False)
        if _chrom_event.has_keys(cw):   # 'chrom_event': the chromatic events alone (pta_engine_chrom_event_add writing its own buffer)
            out["chrom_event"] = self._ce_apply(cw, R, dv.empty((R, self.n_toa)), accumulate=False)
        if self._chrom is not None:
            out["chrom"] = self._chrom_apply(cw, R, r0, dv.empty((R, self.n_toa)), accumulate=False)
        if self._cproc:   # 'common': the sum of the common processes (add_common_process), pta_engine_cproc_add writing its own buffer
            out["common"] = self._cproc_apply(cw, R, r0, dv.empty((R, self.n_toa)), accumulate=False)
        return out

    def stream_to_host(self, total, chunk=480, r0=0):
        """Generator over (first_realisation, host_array[n, n_toa]) covering realisations r0 .. r0+total-1: generation on
        the current stream, device->host copies of the previous chunk on a second stream into two pinned buffers, so the
        PCIe link (2.72 MB per realisation at 68 x 5000) is the only thing waited for.  The yielded array is a view of a
        pinned buffer and is valid ONLY until the generator is resumed: asking for the next chunk immediately queues the copy
        of chunk k+2 into the very buffer chunk k was yielded from - copy the array if it must outlive the next next()."""
        if not self._prepared:
            self.prepare()
        chunk = int(min(chunk, total))
        dev = [dv.empty((chunk, self.n_toa)) for _ in range(2)]
        host = [torch.empty((chunk, self.n_toa), dtype=torch.float64).pin_memory() for _ in range(2)]
        copy_stream = torch.cuda.Stream()
        filled = [torch.cuda.Event(), torch.cuda.Event()]   # generation of buffer b finished
        copied = [torch.cuda.Event(), torch.cuda.Event()]   # its copy to the host finished
        main = torch.cuda.current_stream()
        pending = []                                        # (buffer, first realisation, count) copies in flight
        done = 0
        while done < total or pending:
            if done < total:
                b = (done // chunk) & 1
                n = min(chunk, total - done)
                if done >= 2 * chunk:
                    main.wait_event(copied[b])              # the device buffer is free again
                self.generate(n, r0=r0 + done, out=dev[b][:n])
                filled[b].record(main)
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(filled[b])
                    host[b][:n].copy_(dev[b][:n], non_blocking=True)
                    copied[b].record(copy_stream)
                pending.append((b, r0 + done, n))
                done += n
            if len(pending) == 2 or done >= total:
                b, first, n = pending.pop(0)
                copied[b].synchronize()
                yield first, host[b][:n].numpy()

    # ---------------------------------------------------------------- replay mode ---------------
    def dump_draws(self, r):
        """The normals realisation r uses in generate(), as NumPy arrays in the reference's shapes:
        {'gwb': w[P,Nf] complex, 'rn': [z[K]], 'wn': [(z1[N_a], z2[N_a])], 'ecorr': [z[E_a]], 'chrom': [z[K_c]]}."""
        self._require_reference_draws("dump_draws")
        if not self._prepared:
            self.prepare()
        s = dv.stream_ptr()
        d = {}
        if self.plan.gw_npts:
            Nf = self.grid["Nf"]
            buf = dv.empty((self.P, 2 * Nf))
            for a in range(self.P):
                _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_GWB, a), Nf, 1,
                          ctypes.c_void_p(buf.data_ptr() + 16 * Nf * a), None, 2 * Nf, int(self.rng_fast), s)
            w = buf.cpu().numpy().reshape(self.P, Nf, 2)
            d["gwb"] = w[:, :, 0] + 1j * w[:, :, 1]
        if self.plan.rn_k:
            d["rn"] = []
            for a in range(self.P):
                buf = dv.empty((self.K,))
                _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_RN, a), self.K // 2, 1, dv.ptr(buf), None, self.K, int(self.rng_fast), s)
                d["rn"].append(buf.cpu().numpy())
        if self.plan.wn_a:
            d["wn"] = []
            for a in range(self.P):
                n = int(self.counts[a])
                z1, z2 = dv.empty((n,)), dv.empty((n,))
                _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_WN, a), n, 0, dv.ptr(z1), dv.ptr(z2), n, int(self.rng_fast), s)
                d["wn"].append((z1.cpu().numpy(), z2.cpu().numpy()))
        if self.plan.ecorr_toa:
            d["ecorr"] = []
            for a in range(self.P):
                ne = len(self.ecorrvec[a])
                npair = (ne + 1) // 2
                buf = dv.empty((2 * npair,))
                _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_ECORR, a), npair, 1, dv.ptr(buf), None, 2 * npair, int(self.rng_fast), s)
                d["ecorr"].append(buf.cpu().numpy()[:ne])
        if self._chrom is not None:
            Kc = self._chrom_t["K"]
            d["chrom"] = []
            for a in range(self.P):
                buf = dv.empty((Kc,))
                _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_CHROM, a), Kc // 2, 1, dv.ptr(buf), None, Kc, int(self.rng_fast), s)
                d["chrom"].append(buf.cpu().numpy())
        if self._cproc:   # 'common': per process z [2 n_f, rho], column c major, factor column j minor
            t = self._cproc_t
            d["common"] = []
            for p, (kp, rho) in enumerate(zip(t["kp"], t["rho"])):
                npair = (kp * rho + 1) // 2
                buf = dv.empty((2 * npair,))
                _lib.call("pta_rng_fill_normal", self.seed, r, 1, stream_id(STREAM_CPROC, p), npair, 1, dv.ptr(buf), None, 2 * npair, int(self.rng_fast), s)
                d["common"].append(buf.cpu().numpy()[:kp * rho].reshape(kp, rho))
        return d

    def replay(self, draws_list, per_signal=False):
        """Push caller-supplied draws through the per-signal kernels (replay mode / parity path).

        draws_list: one dict per realisation, shaped like dump_draws().  Returns out[R, n_toa] (device), or with
        per_signal=True a dict of such tensors keyed 'rn', 'chrom', 'gwb', 'wn', 'ecorr', 'det', 'total' (the order 'total' sums them in)."""
        self._require_reference_draws("replay")
        if not self._prepared:
            self.prepare()
        s = dv.stream_ptr()
        R, P, N = len(draws_list), self.P, self.n_toa
        sig = {}
        pl = self.plan
        if pl.rn_k:
            coef = np.zeros((R, P, self.K))
            for r, d in enumerate(draws_list):
                for a in range(P):
                    coef[r, a] = self.rn_amp[a] * d["rn"][a]
            coef_d = dv.f64(coef)
            out = dv.zeros((R, N))
            for a in range(P):
                n = int(self.counts[a])
                _lib.call("pta_rn_synth", ctypes.c_void_p(self.d_Ft.data_ptr() + 8 * int(self.off[a])), N, n, self.K,
                          ctypes.c_void_p(coef_d.data_ptr() + 8 * a * self.K), P * self.K, R,
                          ctypes.c_void_p(out.data_ptr() + 8 * int(self.off[a])), N, 0, s)
            sig["rn"] = out
        if self._chrom is not None:   # the red-noise synthesis on the weighted design matrix
            t = self._chrom_t
            Kc = t["K"]
            coef = np.zeros((R, P, Kc))
            for r, d in enumerate(draws_list):
                for a in range(P):
                    coef[r, a] = t["amp_host"][a] * d["chrom"][a]
            ccoef_d = dv.f64(coef)
            out = dv.zeros((R, N))
            for a in range(P):
                n = int(self.counts[a])
                _lib.call("pta_rn_synth", ctypes.c_void_p(t["Ft"].data_ptr() + 8 * int(self.off[a])), N, n, Kc,
                          ctypes.c_void_p(ccoef_d.data_ptr() + 8 * a * Kc), P * Kc, R,
                          ctypes.c_void_p(out.data_ptr() + 8 * int(self.off[a])), N, 0, s)
            sig["chrom"] = out
        if self._cproc:   # the coefficients on the host from the given draws, then the add kernel writing a buffer of its own
            t = self._cproc_t
            coef = np.zeros((R, P, t["K"]))
            for r, d in enumerate(draws_list):
                for p, (kp, B) in enumerate(zip(t["kp"], t["B_host"])):
                    coef[r, :, :kp] += t["amp_host"][p, :kp][None, :] * (B @ np.asarray(d["common"][p]).T)
            sig["common"] = self._cproc_add_coef(dv.f64(coef), R, dv.zeros((R, N)))
        if pl.gw_npts:
            Nf, npts = self.grid["Nf"], pl.gw_npts
            w = np.zeros((R, P, Nf, 2))
            for r, d in enumerate(draws_list):
                w[r, :, :, 0], w[r, :, :, 1] = d["gwb"].real, d["gwb"].imag
            w_d = dv.f64(w)
            G0, G = dv.empty((R * P, npts)), dv.empty((R * P, npts))
            _lib.call("pta_gwb_idft", dv.ptr(w_d), 2 * Nf, R * P, Nf, dv.ptr(self.d_T), self.ldt, npts, dv.ptr(G0), npts, 1, s)
            _lib.call("pta_gwb_mix", dv.ptr(self.d_M), P, dv.ptr(G0), R, npts, npts, dv.ptr(G), int(self.mix_variant), s)
            out = dv.empty((R, N))
            _lib.call("pta_gwb_interp", dv.ptr(G), npts, P, npts, dv.ptr(self.d_ut), dv.ptr(self.d_toa_s), dv.ptr(self.d_psr_of),
                      dv.ptr(self.d_jlo), N, R, ctypes.c_double(1.0), dv.ptr(out), N, 0, s)
            sig["gwb"] = out
            self._last_G = G
        if pl.wn_a:
            z1 = np.zeros((R, N)); z2 = np.zeros((R, N))
            for r, d in enumerate(draws_list):
                z1[r] = np.concatenate([x[0] for x in d["wn"]]); z2[r] = np.concatenate([x[1] for x in d["wn"]])
            sg, ef, eq = dv.f64(np.concatenate(self.sigma_s)), dv.f64(np.concatenate(self.efacvec)), dv.f64(np.concatenate(self.equadvec))
            z1_d, z2_d = dv.f64(z1), dv.f64(z2)
            out = dv.empty((R, N))
            _lib.call("pta_wn", dv.ptr(sg), dv.ptr(ef), dv.ptr(eq), N, int(self._wn["tnequad"]), dv.ptr(z1_d), dv.ptr(z2_d), N, R,
                      dv.ptr(out), N, 0, s)
            sig["wn"] = out
        if pl.ecorr_toa:
            out = dv.zeros((R, N))
            keep = []                                           # operands stay alive until the single synchronise below
            for a in range(P):
                ne, n = len(self.ecorrvec[a]), int(self.counts[a])
                z = np.zeros((R, ne))
                for r, d in enumerate(draws_list):
                    z[r] = d["ecorr"][a]
                z_d, ep_d, ec_d = dv.f64(z), dv.i32(self.epoch_of[a]), dv.f64(self.ecorrvec[a])
                keep += [z_d, ep_d, ec_d]
                _lib.call("pta_ecorr", dv.ptr(ep_d), dv.ptr(ec_d), n, ne, dv.ptr(z_d), ne, R,
                          ctypes.c_void_p(out.data_ptr() + 8 * int(self.off[a])), N, 0, s)
            torch.cuda.current_stream().synchronize()
            del keep
            sig["ecorr"] = out
        total = dv.zeros((R, N))
        for k in ("rn", "chrom", "common", "gwb", "wn", "ecorr"):
            if k in sig:
                total += sig[k]
        if pl.det:
            sig["det"] = self.d_det.unsqueeze(0).expand(R, N)
            total += self.d_det
        torch.cuda.current_stream().synchronize()
        if per_signal:
            sig["total"] = total
            return sig
        return total

    def inject(self, r, signal_name="engine_realisation"):
        """Write realisation r into the pulsar objects the way the reference's add_* functions do - record the delay in
        ``added_signals`` / ``added_signals_time``, shift the TOAs, rebuild the residuals - but ONCE per pulsar with the summed
        delay (the PINT sink dominates real runs, so it is paid once, not once per signal)."""
        from ._compat import TimeDelta, u
        row = self.generate(1, r0=r)[0].cpu().numpy()
        for a, psr in enumerate(self.psrs):
            dt = row[self.off[a]:self.off[a + 1]] * u.s
            psr.update_added_signals("{}_{}".format(psr.name, signal_name), {"seed": self.seed, "realisation": int(r)}, dt)
            psr.toas.adjust_TOAs(TimeDelta(dt.to("day")))
            psr.update_residuals()
        return row

    # ---------------------------------------------------------------- timing-model projection ---
    def prepare_timing_projection(self, model="spin"):
        """Design matrices M_a (simulate.timing_design_matrix on the IDEAL TOAs: "spin" = offset, F0, F1; "astrometric" = + position,
        proper motion, parallax) and the fit operators Q_a = (M^T W M)^-1 M^T W of every pulsar, W = 1 / sigma^2, on the device
        (K-major over the concatenated TOAs, like Ft).  Realisation independent: computed once."""
        from .simulate import timing_design_matrix
        dv.require_gpu()
        Mt = Qt = None
        for a in range(self.P):
            M, names = timing_design_matrix(self.mjd[a] * 86400.0, model=model)
            w = 1.0 / self.sigma_s[a] ** 2
            # scale the weights (the projection is invariant): sigma ~ 1e-6 s would put M^T W M at 1e12 and lose digits to nothing
            w = w / w.mean()
            A = M.T @ (M * w[:, None])
            Q = np.linalg.solve(A, M.T * w[None, :])
            if Mt is None:
                m = M.shape[1]
                Mt, Qt = np.zeros((m, self.n_toa)), np.zeros((m, self.n_toa))
            Mt[:, self.off[a]:self.off[a + 1]] = M.T
            Qt[:, self.off[a]:self.off[a + 1]] = Q
        self._tm = dict(model=model, m=Mt.shape[0], names=names, Mt=dv.f64(Mt), Qt=dv.f64(Qt), off=dv.i32(self.off), Mt_host=Mt, Qt_host=Qt)
        return self

    def project_timing_model(self, rows, model="spin"):
        """In place: every realisation of ``rows`` ([R, n_toa] device tensor, e.g. the output of generate()) loses what a linearised
        refit of the pulsars' timing models would absorb, r <- r - M (M^T W M)^-1 M^T W r per (realisation, pulsar) - the batched
        counterpart of the reference's fit + residual rebuild through PINT (simulate.py:40-69) for idealised timing models
        (pta_tm_project, one launch).  The weighted-mean subtraction of PINT's default residuals is the one-column special case."""
        if getattr(self, "_tm", None) is None or self._tm["model"] != model:
            self.prepare_timing_projection(model)
        tm = self._tm
        assert rows.dim() == 2 and rows.shape[1] == self.n_toa and rows.stride(1) == 1
        _lib.call("pta_tm_project", dv.ptr(tm["Qt"]), dv.ptr(tm["Mt"]), self.n_toa, tm["m"], dv.ptr(tm["off"]), self.P,
                  ctypes.c_void_p(rows.data_ptr()), rows.stride(0), int(rows.shape[0]), dv.stream_ptr())
        return rows

    def to_enterprise(self, rows, subtract_mean=True, timing_model="spin", fitted=False):
        """enterprise-style pulsar objects for realisations already generated: ``rows`` is a [R, n_toa] tensor / array (e.g. the
        output of generate() or generate_td()); returns R lists of P ``ArrayEnterprisePulsar`` whose ``toas`` are the ideal TOAs
        shifted by the realisation's delay (what the reference's hand-off carries, simulate.py:91-95) and whose ``residuals`` are the
        injected delays with the weighted mean removed (what PINT's Residuals would report for an idealised pulsar, SURVEY.md §8
        a16) - the hand-off of SURVEY.md §8f rank 4 for whole ensembles, without a par/tim round trip.  Works for array-backed,
        PINT-backed and foreign pulsars alike: everything is read from the engine's own copies of the ideal TOAs / errors and the
        pulsar's flag table.  ``fitted=True``: the residuals are POST-FIT - the columns of ``Mmat`` are projected out of every
        realisation on the device (project_timing_model) before the hand-off; the TOAs still carry the full injected delay."""
        from .simulate import ArrayEnterprisePulsar
        from ._position import ra_dec
        if fitted:   # post-fit residuals: the design matrix handed over (Mmat) is projected out on the device, whole ensemble at once
            dev = rows.detach().clone() if hasattr(rows, "detach") else dv.f64(np.atleast_2d(np.asarray(rows)))
            if dev.dim() == 1:
                dev = dev[None, :].contiguous()
            rows = self.project_timing_model(dev, timing_model)
            subtract_mean = False
        arr = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows)
        if arr.ndim == 1:
            arr = arr[None, :]
        meta = []
        for a, psr in enumerate(self.psrs):
            toas = psr.toas
            flags = list(toas.table["flags"].data)
            freq = getattr(toas, "freqs_mhz", None)
            if freq is None:
                try:
                    freq = np.asarray(toas.get_freqs().to("MHz").value, dtype=np.float64)
                except AttributeError:
                    freq = 1440.0
            meta.append((flags, np.asarray(freq, dtype=np.float64) * np.ones(int(self.counts[a])), ra_dec(psr, default=(0.0, 0.0))))
        out = []
        for row in arr:
            psrs = []
            for a, psr in enumerate(self.psrs):
                x = row[self.off[a]:self.off[a + 1]]
                res = x
                if subtract_mean:
                    w = 1.0 / self.sigma_s[a] ** 2
                    res = x - np.sum(x * w) / np.sum(w)
                flags, freq, (ra, dec) = meta[a]
                mjd = self.mjd[a].astype(np.longdouble) + (x / 86400.0).astype(np.longdouble)
                psrs.append(ArrayEnterprisePulsar(psr.name, np.asarray(mjd, dtype=np.float64), res, self.sigma_s[a] * 1e6, freq, flags, ra, dec,
                                                  timing_model=timing_model))
            out.append(psrs)
        return out

    def write_tim_ensemble(self, rows, outdir, r0=0):
        """Batched counterpart of SimulatedPulsar.write_partim (simulate.py:71-77) for array-backed pulsars: one directory
        ``real_<r>/`` per realisation with a Tempo2 tim file per pulsar whose TOAs are the ideal TOAs shifted by the injected
        delay - without touching the pulsar objects (no per-realisation adjust_TOAs / residual rebuild) - and, ONCE (``par/``), the par
        file of every pulsar: the timing models are the same in every realisation."""
        import os
        from .simulate import ArrayTOAs, minimal_par, write_tim
        arr = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows)
        if arr.ndim == 1:
            arr = arr[None, :]
        for psr in self.psrs:
            if not isinstance(psr.toas, ArrayTOAs):
                raise NotImplementedError("write_tim_ensemble needs array-backed pulsars (PINT-backed: use inject() + write_partim)")
        os.makedirs(os.path.join(outdir, "par"), exist_ok=True)
        for psr in self.psrs:
            with open(os.path.join(outdir, "par", f"{psr.name}.par"), "w") as fh:
                fh.write(psr.par_text if getattr(psr, "par_text", None) else minimal_par(psr.name, psr.loc))
        paths = []
        for k, row in enumerate(arr):
            d = os.path.join(outdir, f"real_{r0 + k:06d}")
            os.makedirs(d, exist_ok=True)
            for a, psr in enumerate(self.psrs):
                mjd = psr.toas.mjd0_ld + (row[self.off[a]:self.off[a + 1]] / 86400.0).astype(np.longdouble)
                path = os.path.join(d, f"{psr.name}.tim")
                write_tim(path, psr.name, mjd, psr.toas.errors_us, psr.toas.freqs_mhz, psr.toas.flags)
                paths.append(path)
        return paths

    def split(self, arr):
        """per-pulsar views of an [..., n_toa] array."""
        return [arr[..., self.off[a]:self.off[a + 1]] for a in range(self.P)]
