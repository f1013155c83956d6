"""Cross-correlation optimal statistic (OS) of the ReplicaEngine's realisations, per realisation, on the device.

``prepare_optimal_statistic()`` builds the realisation-independent operands on the host from the noise model ``prepare()`` holds
(pta_replicator_amd/optimal_statistic.py: W_a = S^1/2 F^T P_a^-1, Z_a, den_ab, the ORF weights) and uploads them once;
``optimal_statistic(rows)`` then costs two launches per batch:

    pta_os_project   Y[r, a, :] = W_a r_a             every residual read once (fp64 MFMA)
    pta_os_pairs     A2[r, o] = sum_{a<b} G_o,ab Y_ra . Y_rb / sum G_o^2 den      one workgroup per realisation

and ``generate_os(R)`` runs generate / generate_td / generate(theta=...) chunk by chunk into one reused buffer with the OS behind
each chunk, keeping only the statistics.  A realisation's statistic is bit-identical whatever chunk or row it is computed in.

``prepare_optimal_statistic(matched=True)`` also prepares the OS whose noise model follows theta per realisation (red noise and the
GWB auto-term; white noise, ECORR and the timing model stay fixed): V = U^T P0' and A = U^T P0' U per pulsar, U = [F_rn | F].
``optimal_statistic(rows, theta=...)`` and ``generate_os(R, theta=..., matched=True)`` then run

    pta_os_project         q[r, a, :] = V_a r_a            once per block of <= 64 rows of V
    pta_os_matched_prior   b[r, a, :] = prior variances of theta over the mean white-noise variance
    pta_os_matched_solve   X_ra = W_a(theta_r) r_a, Z_ra = Z_a(theta_r)      one workgroup per (realisation, pulsar)
    pta_os_matched_pairs   A2, sigma (and rho, sigma_pair) per realisation

with sigma (and sigma_pair) per realisation.

``optimal_statistic_spectrum(rows)`` and ``generate_os_spectrum(R)`` return the per-frequency statistic instead: the cross-correlated
power of every Fourier bin per ORF, a2 = F^-1 b ("full") or b_k / F_kk ("narrowband"), without a spectral shape.  The front is the
same (pta_os_project, or project / prior / solve with theta); the pair stage is pta_os_pairs_pf (F fixed, its inverse prepared on the
host at the first call) or pta_os_matched_pairs_pf (F accumulated and solved per realisation in LDS).

The argument checks, the host noise model, the rows and state checks, theta on the device, the blocked projection and the chunked
generation loop with its rows buffer are engine_stats.StatisticsMixin's, shared with the likelihood and the F-statistic.
"""
import ctypes

import numpy as np

from . import _chrom, _cproc, _hyper, _lib, device as dv
from . import optimal_statistic as ost
from . import red_noise as rn
from . import spharmORFbasis as anis
from ._position import ra_dec
from .engine_stats import StatisticsMixin, check_components, check_timing_model


class OptimalStatisticMixin(StatisticsMixin):
    def prepare_optimal_statistic(self, components=14, gamma=13. / 3., orfs=ost.ORF_NAMES, timing_model="spin", gwb_auto=None, matched=False,
                                  anisotropy_lmax=None):
        """W, Z, den and ORF weights of the array under the configured noise model (white noise + ECORR + red noise, optionally the
        GWB auto-term), uploaded once.

        components: n_f = 1 .. 32 frequencies k / T (T = span of the whole array); gamma: spectral index of the unit spectrum;
        orfs: names "hd", "monopole", "dipole" or [P, P] arrays (at most 8); timing_model: "spin", "astrometric" or None;
        gwb_auto: None = the configured GWB amplitude if a GWB is set, else no GW term in C_a; a float = that log10_A; False = off.
        matched: also prepare the OS under per-realisation noise parameters (optimal_statistic(theta=...), generate_os(matched=True)):
        K = red-noise columns + 2 n_f <= 128.
        anisotropy_lmax = L (0 .. 8): also prepare the JOINT fit of the (L+1)^2 spherical-harmonic basis ORFs Gamma_k,ab =
        basis[k][a, b] (spharmORFbasis.correlated_basis, the code the generation's ORF = 2 sum_k c_k basis[k] is built from, so that
        E[rho_ab] = A^2 sum_k c_k Gamma_k,ab exactly): optimal_statistic(rows) and generate_os(R) then also return a2clm [R, n_lm], the
        estimates of A^2 c_lm (a2clm[:, 0] / sqrt(4 pi) is the isotropic A^2 of the joint fit), clm_sigma [n_lm] and clm_cov
        [n_lm, n_lm] (optimal_statistic.joint_weights; pta_os_pairs with the joint weights, 8 rows per call).  Needs at least
        (L+1)^2 pairs.  The fixed-noise statistic only: not together with matched=True, and the per-frequency OS does not carry it."""
        check_components(components)
        if matched:
            _chrom.refuse_matched(self._chrom, "prepare_optimal_statistic(matched=True)")
            _cproc.refuse_matched(self._cproc, "prepare_optimal_statistic(matched=True)")
        if anisotropy_lmax is not None:
            if isinstance(anisotropy_lmax, bool) or not isinstance(anisotropy_lmax, (int, np.integer)) or not 0 <= anisotropy_lmax <= anis.LMAX_SUPPORTED:
                raise ValueError(f"anisotropy_lmax={anisotropy_lmax!r}: an integer 0 .. {anis.LMAX_SUPPORTED}")
            if matched:
                raise ValueError("anisotropy_lmax: the joint spherical-harmonic fit belongs to the fixed-noise statistic (not with matched=True)")
            if self.P * (self.P - 1) // 2 < (int(anisotropy_lmax) + 1) ** 2:
                raise ValueError(f"anisotropy_lmax={anisotropy_lmax}: the joint fit of {(int(anisotropy_lmax) + 1) ** 2} ORFs needs at least as many "
                                 f"pulsar pairs, got {self.P * (self.P - 1) // 2}")
        check_timing_model(timing_model)
        orfs = tuple(orfs) if not isinstance(orfs, str) else (orfs,)
        if not 1 <= len(orfs) <= 8:
            raise ValueError(f"{len(orfs)} ORFs: one call evaluates 1 .. 8")
        for o in orfs:
            if isinstance(o, str) and o not in ost.ORF_NAMES:
                raise ValueError(f"unknown ORF {o!r}: expected one of {ost.ORF_NAMES} or a [P, P] array")
            if not isinstance(o, str) and np.shape(o) != (self.P, self.P):
                raise ValueError(f"a user ORF must be a finite [{self.P}, {self.P}] array, got shape {np.shape(o)}")
        if self.P < 2:
            raise ValueError("the cross-correlation OS needs at least two pulsars")
        self._stats_need_noise("the OS")
        gw_lA = self._stats_gwb_auto(gwb_auto)
        amp2 = 0.0 if gw_lA is None else 10.0 ** (2 * gw_lA)
        K_rn = 2 * self._rn["components"] if self._rn is not None else 0
        if matched and K_rn + 2 * int(components) > _lib.OSM_KMAX:
            raise ValueError(f"matched=True: K = {K_rn} red-noise columns + {2 * int(components)} OS columns exceeds the kernel limit of "
                             f"{_lib.OSM_KMAX}")
        toas, sigma2, epoch_of, ecorr, F_rn, phi_rn, M = self._stats_noise_model(timing_model)
        pos = []
        for p in self.psrs:
            ra, dec = ra_dec(p, default=(0.0, 0.0))
            pos.append([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)])
        plan = ost.prepare(toas, sigma2, np.array(pos), components=int(components), gamma=float(gamma), orfs=orfs, epoch_of=epoch_of,
                           ecorr=ecorr, F_rn=F_rn, phi_rn=phi_rn, gw_amp2=amp2, M=M)
        self._os = dict(plan=plan, engine_plan=self.plan, C=plan.C, n_orf=len(plan.names), names=plan.names,
                        Wt=dv.f64(plan.Wt()), off=dv.i32(self.off), pa=dv.i32(plan.pair_a), pb=dv.i32(plan.pair_b),
                        wt=dv.f64(plan.weights), den=dv.f64(plan.den), sigma=dv.f64(plan.sigma), sigma_pair=dv.f64(plan.sigma_pair),
                        zeta=dv.f64(plan.zeta), pairs=dv.i64(np.stack([plan.pair_a, plan.pair_b], axis=1)), Y=None, matched=None, aniso=None)
        if anisotropy_lmax is not None:
            basis = anis.correlated_basis_device(rn.pulsar_locations(self.psrs), int(anisotropy_lmax)).cpu().numpy()
            Wj, cov, sig = ost.joint_weights(basis[:, plan.pair_a, plan.pair_b], plan.den)
            self._os["aniso"] = dict(lmax=int(anisotropy_lmax), n_lm=len(sig), Wj_host=Wj, Wj=dv.f64(Wj), cov=dv.f64(cov), sigma=dv.f64(sig))
        if matched:
            mp = ost.prepare_matched(toas, sigma2, np.array(pos), components=int(components), gamma=float(gamma), orfs=orfs,
                                     epoch_of=epoch_of, ecorr=ecorr, F_rn=F_rn, M=M)
            m = dict(plan=mp, K=mp.K, K_rn=mp.K_rn, nz=mp.C * (mp.C + 1) // 2, Vt=dv.f64(mp.Vt()), A=dv.f64(mp.A), s=dv.f64(mp.s), S=dv.f64(mp.S),
                     G=dv.f64(mp.G), G2=dv.f64(mp.G ** 2), T=mp.T, gw=None if gw_lA is None else (gw_lA, float(gamma)), ws=None, rn_phi=None)
            if mp.K_rn:
                m["rn_phi"] = dv.f64(self.rn_amp ** 2)
            self._os["matched"] = m
        return self

    def _os_state(self, what):
        return self._stats_state("_os", "the optimal statistic", "prepare_optimal_statistic", what)

    def optimal_statistic(self, rows, pairs=False, theta=None):
        """OS of every realisation of rows [R, n_toa] (a float64 device tensor with unit column stride: any output of generate,
        generate_td, generate_sampled, or the caller's own residuals).  Returns a dict of device tensors: A2 [R, n_orf], snr [R, n_orf],
        sigma [n_orf], names (list); with pairs=True also rho [R, n_pairs] (= num / den), sigma_pair [n_pairs], zeta [n_pairs] and
        pairs [n_pairs, 2] (a < b, row-major upper triangle).  Prepared with anisotropy_lmax: also a2clm [R, n_lm], clm_sigma [n_lm] and
        clm_cov [n_lm, n_lm], the joint spherical-harmonic fit (not with theta: ValueError).

        theta (needs prepare_optimal_statistic(matched=True)): per-realisation noise parameters as generate(theta=...) takes them;
        row r is then weighted with the noise model of theta[r] (keys not given and NaN red-noise amplitudes: as configured / as
        prepared; cw_* keys are ignored).  sigma is then [R, n_orf] and sigma_pair [R, n_pairs].  With gwb_log10_hc [R, M] (an engine
        configured with a userSpec, the statistic prepared with the GW auto-term) the GW auto-term of row r follows its own spectrum;
        the broadband template S(gamma) stays the prepared one."""
        _chrom.refuse_noise_model(theta)
        _cproc.refuse_noise_model(theta)
        st = self._os_state("optimal_statistic")
        R = self._stats_check_rows(rows)
        if theta is not None:
            self._os_no_aniso(st, "optimal_statistic(theta=...)")
            dev = self._os_matched_theta(st, theta, R, "optimal_statistic")
            out = self._os_matched_out(st, R, pairs)
            step = self._os_matched_chunk(st, R, with_rows=False)
            for lo in range(0, R, step):
                self._os_matched_launch(rows[lo:lo + step], min(step, R - lo), dev, lo, out)
            return self._os_matched_result(st, out)
        out = {"A2": dv.empty((R, st["n_orf"])), "rho": dv.empty((R, len(st["plan"].den))) if pairs else None}
        a2clm = self._os_aniso_out(st, R)
        self._os_launch(rows, R, out["A2"], out["rho"], a2clm)
        return self._os_result(st, out["A2"], out["rho"], a2clm)

    def _os_result(self, st, A2, rho, a2clm=None):
        res = {"A2": A2, "snr": A2 / st["sigma"], "sigma": st["sigma"], "names": list(st["names"])}
        if rho is not None:
            res.update(rho=rho, sigma_pair=st["sigma_pair"], zeta=st["zeta"], pairs=st["pairs"])
        if a2clm is not None:
            res.update(a2clm=a2clm, clm_sigma=st["aniso"]["sigma"], clm_cov=st["aniso"]["cov"])
        return res

    def _os_aniso_out(self, st, R):
        return None if st["aniso"] is None else dv.empty((R, st["aniso"]["n_lm"]))

    def _os_no_aniso(self, st, what):
        if st["aniso"] is not None:
            raise ValueError(f"{what}: the statistic was prepared with anisotropy_lmax, and the joint spherical-harmonic fit (a2clm) belongs "
                             "to the fixed-noise statistic alone: prepare without it")

    def _os_project(self, rows, R):
        """pta_os_project of rows [R, n_toa] into the reused Y buffer [>= R, P * C], on the current stream"""
        st = self._os
        P, C = self.P, st["C"]
        if st["Y"] is None or st["Y"].shape[0] < R:
            st["Y"] = dv.empty((R, P * C))
        self._stats_project(st["Wt"], C, st["off"], rows, R, st["Y"])
        return st["Y"]

    def _os_launch(self, rows, R, A2, rho, a2clm=None):
        """pta_os_project into the reused Y buffer, then pta_os_pairs into A2 (and rho) - both on the current stream; a2clm [R, n_lm]:
        then pta_os_pairs again with the joint weights, _lib.OS_NORF rows of them per call"""
        st = self._os
        P, C = self.P, st["C"]
        Y = self._os_project(rows, R)
        s = dv.stream_ptr()
        npairs = len(st["plan"].den)
        _lib.call("pta_os_pairs", dv.ptr(Y), P * C, P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(st["wt"]), st["n_orf"],
                  ctypes.c_void_p(A2.data_ptr()), A2.stride(0), dv.ptr(st["den"]) if rho is not None else None,
                  ctypes.c_void_p(rho.data_ptr()) if rho is not None else None, rho.stride(0) if rho is not None else 0, s)
        if a2clm is not None:
            Wj = st["aniso"]["Wj"]
            for k0 in range(0, Wj.shape[0], _lib.OS_NORF):
                _lib.call("pta_os_pairs", dv.ptr(Y), P * C, P, C, R, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.row_ptr(Wj, k0),
                          min(_lib.OS_NORF, Wj.shape[0] - k0), ctypes.c_void_p(a2clm.data_ptr() + 8 * k0), a2clm.stride(0), None, None, 0, s)

    def generate_os(self, R, r0=0, theta=None, td=False, chunk=1024, pairs=False, matched=False):
        """OS of realisations r0 .. r0+R-1, generated chunk by chunk into one reused [chunk, n_toa] buffer (generate, generate_td with
        td=True, or generate(theta=...) with theta = per-realisation parameters of the R realisations, e.g. sample_theta(R, r0)); only
        the statistics are kept.  Same results as optimal_statistic(generate(R, r0, ...)), bit for bit, whatever the chunk.  The chunk
        is cut so that the buffer stays within workspace_bytes.  With white-noise keys (wn_efac, wn_log10_equad, wn_log10_ecorr) in theta
        the realisations carry them and the statistic weights with the configured white noise, as it does for red-noise keys.

        matched=True (needs theta and prepare_optimal_statistic(matched=True)): every chunk's statistic is evaluated under the theta
        it was generated with - optimal_statistic(generate(R, r0, theta=theta), theta=theta), bit for bit; rows, q, b, X and Z of a
        chunk stay within workspace_bytes.  The matched noise model ignores theta's gwb_clm as it ignores cw_*: its GW auto-term stays the
        isotropic one; it refuses the white-noise keys (its per-TOA weights are built once, from the configured white noise).  Prepared
        with anisotropy_lmax the result also has a2clm, clm_sigma and clm_cov (not with matched=True)."""
        if td:
            _chrom.refuse_td(self._chrom, "generate_os(td=True)")
            _cproc.refuse_td(self._cproc, "generate_os(td=True)")
        if matched:
            _chrom.refuse_noise_model(theta)
            _cproc.refuse_noise_model(theta)
        st = self._os_state("generate_os")
        R, r0, chunk = int(R), int(r0), int(chunk)
        if R < 1 or chunk < 1 or r0 < 0:
            raise ValueError(f"generate_os: R={R}, chunk={chunk} must be >= 1 and r0={r0} >= 0")
        hyper, cw = self._theta_parts(theta, R, td=td)   # all of theta, before the first chunk is launched
        mdev = None
        if matched:
            self._os_no_aniso(st, "generate_os(matched=True)")
            if theta is None:
                raise ValueError("generate_os: matched=True needs theta (the noise parameters every realisation is evaluated under)")
            mdev = self._os_matched_theta(st, theta, R, "generate_os")
            chunk = min(chunk, self._os_matched_chunk(st, R, with_rows=True))
        A2 = rho = mout = None
        if matched:
            mout = self._os_matched_out(st, R, pairs)
        else:
            A2 = dv.empty((R, st["n_orf"]))
            rho = dv.empty((R, len(st["plan"].den))) if pairs else None
        a2clm = None if matched else self._os_aniso_out(st, R)
        for lo, n, rows in self._os_generate_chunks("generate_os", st, R, r0, hyper, cw, td, chunk):
            if matched:
                self._os_matched_launch(rows, n, mdev, lo, mout)
            else:
                self._os_launch(rows, n, A2[lo:lo + n], None if rho is None else rho[lo:lo + n], None if a2clm is None else a2clm[lo:lo + n])
        return self._os_matched_result(st, mout) if matched else self._os_result(st, A2, rho, a2clm)

    def _os_generate_chunks(self, what, st, R, r0, hyper, cw, td, chunk):
        """_stats_generate_chunks with the chunk cut so that rows and Y stay within workspace_bytes"""
        per_real = 8 * (self.n_toa + self.P * st["C"])
        chunk = max(1, min(chunk, R, int(self.workspace_bytes) // per_real))
        return self._stats_generate_chunks(lambda: self._os_state(what), R, r0, hyper, cw, td, chunk)

    # ---- the OS under per-realisation noise parameters ----
    def _os_matched_theta(self, st, theta, R, what):
        """theta validated as the OS's noise model (_hyper.check_theta_os) -> the device tensors of _stats_theta_device.  With
        gwb_log10_hc [R, M] (an engine configured with a userSpec; needs the GW auto-term) the GW columns of realisation r are weighted
        with its own spectrum (pta_os_matched_prior_spec) instead of (gwb_log10_A, gwb_gamma).  The broadband template S(gamma) of the
        statistic stays the prepared one."""
        m = st["matched"]
        if m is None:
            raise ValueError(f"{what}: theta needs prepare_optimal_statistic(matched=True)")
        th = _hyper.check_theta_os(theta, R, self.P, self._rn, m["gw"] is not None, gw=self._gw)
        return self._stats_theta_device(m["gw"], m["K_rn"], th, R)

    def _os_matched_chunk(self, st, R, with_rows):
        """realisations per launch sequence: q and b [P, K], X [P, C], Z [P, C (C + 1) / 2] (and the generated rows) of a chunk within
        workspace_bytes"""
        m = st["matched"]
        per_real = 8 * (self.P * (2 * m["K"] + st["C"] + m["nz"]) + (self.n_toa if with_rows else 0))
        return max(1, min(R, int(self.workspace_bytes) // per_real))

    def _os_matched_out(self, st, R, pairs):
        npairs = len(st["plan"].den)
        return {"A2": dv.empty((R, st["n_orf"])), "sigma": dv.empty((R, st["n_orf"])), "rho": dv.empty((R, npairs)) if pairs else None,
                "sigma_pair": dv.empty((R, npairs)) if pairs else None}

    def _os_matched_result(self, st, out):
        res = {"A2": out["A2"], "snr": out["A2"] / out["sigma"], "sigma": out["sigma"], "names": list(st["names"])}
        if out["rho"] is not None:
            res.update(rho=out["rho"], sigma_pair=out["sigma_pair"], zeta=st["zeta"], pairs=st["pairs"])
        return res

    def _os_matched_front(self, rows, n, dev, lo):
        """rows [n, n_toa] = realisations lo .. lo+n-1 of theta `dev` -> the workspace with X [n, P C] and packed Z [n, P nz]:
        pta_os_project per block of 64 rows of V, pta_os_matched_prior, pta_os_matched_solve, all on the current stream"""
        st = self._os
        m = st["matched"]
        P, C, K, K_rn, nz = self.P, st["C"], m["K"], m["K_rn"], m["nz"]
        ws = m["ws"]
        if ws is None or ws["n"] < n:
            m["ws"] = None
            ws = m["ws"] = dict(n=n, q=dv.empty((n, P * K)), b=dv.empty((n, P * K)), X=dv.empty((n, P * C)), Z=dv.empty((n, P * nz)))
        s = dv.stream_ptr()
        self._stats_project(m["Vt"], K, st["off"], rows, n, ws["q"])
        at = dv.row_ptr
        hy = self._hyper_tables() if K_rn else {}
        if dev["gw_log10_hc"] is not None:
            sp = self._os_matched_spec_tables(m, C)
            M = dev["gw_log10_hc"].shape[1]
            _lib.call("pta_os_matched_prior_spec", n, P, K_rn, C, dv.ptr(hy["rn_f"]) if K_rn else None, dv.ptr(hy["rn_tspan"]) if K_rn else None,
                      dv.ptr(m["rn_phi"]) if K_rn else None, at(dev["rn_log10_A"], lo), at(dev["rn_gamma"], lo), m["T"], dv.ptr(sp[0]), dv.ptr(sp[1]),
                      dv.ptr(sp[2]), M, at(dev["gw_log10_hc"], lo), M, dv.ptr(m["s"]), dv.ptr(ws["b"]), s)
        else:
            _lib.call("pta_os_matched_prior", n, P, K_rn, C, dv.ptr(hy["rn_f"]) if K_rn else None, dv.ptr(hy["rn_tspan"]) if K_rn else None,
                      dv.ptr(m["rn_phi"]) if K_rn else None, at(dev["rn_log10_A"], lo), at(dev["rn_gamma"], lo), m["T"], at(dev["gw_log10_A"], lo),
                      at(dev["gw_gamma"], lo), dv.ptr(m["s"]), dv.ptr(ws["b"]), s)
        _lib.call("pta_os_matched_solve", dv.ptr(m["A"]), P, K, C, n, dv.ptr(ws["b"]), dv.ptr(ws["q"]), P * K, _lib.OS_CMAX, dv.ptr(m["S"]), dv.ptr(m["s"]),
                  dv.ptr(ws["X"]), dv.ptr(ws["Z"]), s)
        self._os_theta_keep = dev   # the launches above read these buffers asynchronously
        return ws

    def _os_matched_spec_tables(self, m, C):
        """(seg, dx, dxp) on the device for the C / 2 frequencies k / T of the statistic against the nodes of the configured userSpec
        (_hyper.spec_tables), built at the first use and kept with the userSpec they were built from"""
        U = self._gw["userSpec"]
        sp = m.get("spec")
        if sp is None or sp[3] is not U:
            _, xp = _hyper.spec_nodes(U)
            seg, dx, dxp = _hyper.spec_tables(np.arange(1, C // 2 + 1) / m["T"], xp)
            sp = m["spec"] = (dv.i32(seg), dv.f64(dx), dv.f64(dxp), U)
        return sp

    def _os_matched_launch(self, rows, n, dev, lo, out):
        """_os_matched_front, then pta_os_matched_pairs into rows lo .. of out"""
        st = self._os
        m = st["matched"]
        ws = self._os_matched_front(rows, n, dev, lo)
        npairs = len(st["plan"].den)
        A2, sg, rho, sp = out["A2"], out["sigma"], out["rho"], out["sigma_pair"]
        row = dv.row_ptr
        _lib.call("pta_os_matched_pairs", dv.ptr(ws["X"]), dv.ptr(ws["Z"]), self.P, st["C"], n, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(m["G"]),
                  dv.ptr(m["G2"]), st["n_orf"], row(A2, lo), A2.stride(0), row(sg, lo), sg.stride(0), row(rho, lo), row(sp, lo),
                  rho.stride(0) if rho is not None else 0, dv.stream_ptr())

    # ---- the per-frequency OS: the spectrum per realisation ----
    def _os_spectrum_check(self, what, st, mode, theta, matched):
        """the refusals shared by the two entry points, in their documented order -> the mode flag of the kernels"""
        if mode not in ost.SPECTRUM_MODES:
            raise ValueError(f"{what}: mode={mode!r} must be one of {ost.SPECTRUM_MODES}")
        if theta is not None and matched and st["matched"] is None:
            raise ValueError(f"{what}: theta needs prepare_optimal_statistic(matched=True)")
        if matched and theta is None:
            raise ValueError(f"{what}: matched=True needs theta (the noise parameters every realisation is evaluated under)")
        return ost.SPECTRUM_MODES.index(mode)

    def _os_spectrum_state(self, st):
        """the fixed-noise operands of the per-frequency OS, built on the host at the first spectrum call: F [n_orf, n_f, n_f], F^-1 and
        sigma of both modes, the template S_k and the frequencies"""
        sp = st.get("spectrum")
        if sp is None:
            plan = st["plan"]
            F = ost.spectrum_fisher(plan)
            nf = F.shape[-1]
            # right-hand sides e_j [n_f, 1, n_f] against F [n_orf, n_f, n_f] broadcast to x[j, o, :] = F_o^-1 e_j; F^-1[o, k, j] = x[j, o, k]
            Finv = ost.spectrum_solve(F, np.eye(nf)[:, None, :], "full")[0].transpose(1, 2, 0)
            sp = st["spectrum"] = dict(F=dv.f64(F), op=(dv.f64(Finv), dv.f64(1.0 / np.diagonal(F, axis1=1, axis2=2))),
                                       sigma=tuple(dv.f64(ost.spectrum_solve(F, np.zeros(nf), mode)[1]) for mode in ost.SPECTRUM_MODES),
                                       G=dv.f64(plan.G))
        return sp

    def _os_spectrum_axes(self, st):
        """(S_k [n_f], f_k [n_f]) on the device: the unit template per bin and the frequencies, the same for the fixed and the matched path"""
        ax = st.get("spectrum_axes")
        if ax is None:
            plan = st["plan"]
            ax = st["spectrum_axes"] = (dv.f64(plan.S[0::2]), dv.f64(np.arange(1, plan.C // 2 + 1) / plan.T))
        return ax

    def _os_spectrum_out(self, st, R, matched, fisher):
        nf = st["C"] // 2
        return {"a2": dv.empty((R, st["n_orf"], nf)), "sigma": dv.empty((R, st["n_orf"], nf)) if matched else None,
                "fisher": dv.empty((R, st["n_orf"], nf, nf)) if matched and fisher else None}

    def _os_spectrum_launch(self, rows, n, mode, dev, lo, out):
        """the per-frequency OS of rows [n, n_toa] into rows lo .. of out: pta_os_project + pta_os_pairs_pf, or with theta `dev` the
        front of the matched OS + pta_os_matched_pairs_pf"""
        st = self._os
        P, C, n_orf = self.P, st["C"], st["n_orf"]
        npairs = len(st["plan"].den)
        row = dv.row_ptr
        a2 = out["a2"]
        if dev is None:
            sp = self._os_spectrum_state(st)
            Y = self._os_project(rows, n)
            _lib.call("pta_os_pairs_pf", dv.ptr(Y), P * C, P, C, n, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(sp["G"]), n_orf,
                      dv.ptr(sp["op"][mode]), mode, row(a2, lo), a2.stride(0), dv.stream_ptr())
            return
        m = st["matched"]
        ws = self._os_matched_front(rows, n, dev, lo)
        sg, fi = out["sigma"], out["fisher"]
        _lib.call("pta_os_matched_pairs_pf", dv.ptr(ws["X"]), dv.ptr(ws["Z"]), P, C, n, dv.ptr(st["pa"]), dv.ptr(st["pb"]), npairs, dv.ptr(m["G"]),
                  dv.ptr(m["G2"]), n_orf, mode, row(a2, lo), a2.stride(0), row(sg, lo), sg.stride(0), row(fi, lo), fi.stride(0) if fi is not None else 0,
                  dv.stream_ptr())

    def _os_spectrum_result(self, st, out, mode, matched, fisher):
        Sk, freqs = self._os_spectrum_axes(st)
        if matched:
            sigma = out["sigma"]
        else:
            sp = self._os_spectrum_state(st)
            sigma = sp["sigma"][mode]
        a2 = out["a2"]
        res = {"a2": a2, "sigma": sigma, "snr": a2 / sigma, "phi": a2 * Sk, "phi_sigma": (sigma * Sk).expand(a2.shape), "freqs": freqs,
               "names": list(st["names"])}
        if fisher:
            res["fisher"] = out["fisher"] if matched else sp["F"]
        return res

    def optimal_statistic_spectrum(self, rows, theta=None, mode="full", fisher=False):
        """Per-frequency OS of every realisation of rows [R, n_toa] (as optimal_statistic takes them): the cross-correlated power of every
        Fourier bin f_k = (k + 1) / T per ORF, without a spectral shape.  Returns a dict of device tensors: a2 [R, n_orf, n_f] (the bin's
        GW variance over the unit template: A^2 in every bin if the data follow the template), sigma [n_orf, n_f], snr = a2 / sigma,
        phi = a2 S_k and phi_sigma = sigma S_k (the variance of one sin / cos coefficient [s^2]), freqs [n_f], names; with fisher=True
        also fisher [n_orf, n_f, n_f].

        mode "full": a2 = F^-1 b with the coupling between the bins, sigma_k = sqrt((F^-1)_kk); "narrowband": a2_k = b_k / F_kk,
        sigma_k = F_kk^-1/2.  theta (needs prepare_optimal_statistic(matched=True)): as optimal_statistic's; F then follows theta per
        realisation, sigma is [R, n_orf, n_f] and fisher [R, n_orf, n_f, n_f]."""
        what = "optimal_statistic_spectrum"
        st = self._os_state(what)
        mode = self._os_spectrum_check(what, st, mode, theta, theta is not None)
        R = self._stats_check_rows(rows)
        matched = theta is not None
        if not matched:
            self._os_spectrum_state(st)
            out = self._os_spectrum_out(st, R, False, fisher)
            self._os_spectrum_launch(rows, R, mode, None, 0, out)
            return self._os_spectrum_result(st, out, mode, False, fisher)
        dev = self._os_matched_theta(st, theta, R, what)
        out = self._os_spectrum_out(st, R, True, fisher)
        step = self._os_matched_chunk(st, R, with_rows=False)
        for lo in range(0, R, step):
            self._os_spectrum_launch(rows[lo:lo + step], min(step, R - lo), mode, dev, lo, out)
        return self._os_spectrum_result(st, out, mode, True, fisher)

    def generate_os_spectrum(self, R, r0=0, theta=None, td=False, chunk=1024, matched=False, mode="full", fisher=False):
        """Per-frequency OS of realisations r0 .. r0+R-1, generated chunk by chunk as generate_os does; only the statistics are kept.
        Same results as optimal_statistic_spectrum(generate(R, r0, ...)), bit for bit, whatever the chunk; with matched=True (needs
        theta) every chunk is evaluated under the theta it was generated with."""
        what = "generate_os_spectrum"
        st = self._os_state(what)
        R, r0, chunk = int(R), int(r0), int(chunk)
        if R < 1 or chunk < 1 or r0 < 0:
            raise ValueError(f"{what}: R={R}, chunk={chunk} must be >= 1 and r0={r0} >= 0")
        mode = self._os_spectrum_check(what, st, mode, theta, matched)
        hyper, cw = self._theta_parts(theta, R, td=td)   # all of theta, before the first chunk is launched
        mdev = None
        if matched:
            mdev = self._os_matched_theta(st, theta, R, what)
            chunk = min(chunk, self._os_matched_chunk(st, R, with_rows=True))
        else:
            self._os_spectrum_state(st)
        out = self._os_spectrum_out(st, R, matched, fisher)
        for lo, n, rows in self._os_generate_chunks(what, st, R, r0, hyper, cw, td, chunk):
            self._os_spectrum_launch(rows, n, mode, mdev, lo, out)
        return self._os_spectrum_result(st, out, mode, matched, fisher)
