"""CPU tests of the host side of the boundary: native epoch bucketing, host-side scalar formulas, the array-backed
pulsar container, error conventions.  (No GPU: nothing here launches a kernel.)"""
import numpy as np
import pytest

from helpers import load, mjd_ld
from oracle import pta_oracle as po


def test_native_quantize_matches_reference_structure():
    from pta_replicator_amd.white_noise import epoch_map
    z = load("c2_b1855.npz")
    mjd = (z["mjd_hi"].astype(np.longdouble) + z["mjd_lo"].astype(np.longdouble)).astype(np.float64)
    toa_flags = z["backends"][z["flag_index"]]
    epoch_of, first = epoch_map(mjd, 0.1)   # real, unsorted tim file
    assert np.array_equal(epoch_of, z["cg01_epoch_of"])
    assert np.array_equal(toa_flags[first], z["cg01_aveflags"])
    epoch_of, first = epoch_map(mjd, 1.0 / 86400.0)
    assert len(first) == int(z["cg1s_n_epochs"]) and np.array_equal(epoch_of, z["cg1s_epoch_of"])


@pytest.mark.parametrize("n,dt", [(1, 0.1), (2, 0.1), (1000, 0.05), (5000, 0.1), (777, 10.0)])
def test_native_quantize_matches_oracle(n, dt):
    from pta_replicator_amd.white_noise import epoch_map, quantize_fast
    rng = np.random.default_rng(n)
    t = rng.uniform(53000, 53000 + n * 0.07, n)
    if n > 10:
        t[5] = t[6]  # a tie
    epoch_of, first = epoch_map(t, dt)
    eo, ne, fo, ave = po.quantize(t, dt=dt)
    assert np.array_equal(epoch_of, eo) and np.array_equal(first, fo)
    avetoas, U = quantize_fast(t, dt=dt)
    assert U.shape == (n, ne) and np.all(U.sum(axis=1) == 1) and np.allclose(avetoas, ave)
    assert np.array_equal(np.argmax(U, axis=1), eo)


def test_quantize_stable_sort_path_and_bad_arguments():
    import ctypes
    from pta_replicator_amd import _lib, device as dv
    t = np.array([3.0, 1.0, 1.04, 2.0, 1.11, 3.05])
    eo = np.empty(6, dtype=np.int32); fi = np.empty(6, dtype=np.int32); ne = ctypes.c_int(0)
    _lib.call("pta_quantize_epochs", dv.hptr(t), 6, 0.1, None, dv.hptr(eo), dv.hptr(fi), ctypes.byref(ne))
    assert ne.value == 4 and list(eo) == [3, 0, 0, 2, 1, 3] and list(fi[:4]) == [1, 4, 3, 0]
    bad = np.array([0, 1, 2, 3, 4, 99], dtype=np.int64)
    with pytest.raises(_lib.PtaError):
        _lib.call("pta_quantize_epochs", dv.hptr(t), 6, 0.1, dv.hptr(bad), dv.hptr(eo), dv.hptr(fi), ctypes.byref(ne))


def _array_psrs(z, prefix, P):
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    out = []
    for i in range(P):
        p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, prefix, i), z[f"{prefix}err_us_{i}"]), name=str(z[prefix + "names"][i]),
                            loc={"RAJ": float(z[prefix + "raj_hours"][i]), "DECJ": float(z[prefix + "decj_deg"][i])})
        make_ideal(p)
        out.append(p)
    return out


@pytest.mark.parametrize("tag", ["raw_", "nudged_"])
def test_gwb_grid_knife_edge_is_reproduced_on_the_host(tag):
    """Nf = 3001 on the raw tim-file MJDs, 3000 after a 1 us nudge: computed with the reference's
    own NumPy expressions, never re-derived on the device."""
    from pta_replicator_amd.red_noise import gwb_spectrum, gwb_time_grid
    z = load("c1_small.npz")
    psrs = _array_psrs(z, tag, 3)
    grid = gwb_time_grid(psrs)
    assert grid["Nf"] == int(z[tag + "Nf"])
    og = po.gwb_grid([float(mjd_ld(z, tag, i).min()) for i in range(3)], [float(mjd_ld(z, tag, i).max()) for i in range(3)])
    assert np.array_equal(grid["f"], og["f"]) and np.array_equal(grid["ut"], og["ut"]) and grid["dt"] == og["dt"]
    C = gwb_spectrum(grid["f"], grid["dur"], 10, -14, 4.33)
    assert np.array_equal(C, po.gwb_spectrum(og["f"], og["dur"], 10, -14, 4.33))


def test_gwb_spectrum_branches_match_oracle():
    from pta_replicator_amd.red_noise import gwb_spectrum
    z = load("variants.npz")
    f = np.arange(0, 1e-6, 3e-10); f[0] = f[1]
    for kw in (dict(turnover=True, f0=3e-9, beta=1.2, power=2.0), dict(userSpec=z["userSpec"]), dict()):
        a = gwb_spectrum(f, 3e8, 10, -14.2, 13. / 3., **kw)
        b = po.gwb_spectrum(f, 3e8, 10, -14.2, 13. / 3., **kw)
        assert np.max(np.abs(a - b) / b) < 1e-13
    # an UNSORTED user spectrum: the reference's scipy interp1d sorts the points (assume_sorted=False) before interpolating
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(z["userSpec"]))
    a = gwb_spectrum(f, 3e8, 10, -14.2, 13. / 3., userSpec=z["userSpec"][perm])
    b = gwb_spectrum(f, 3e8, 10, -14.2, 13. / 3., userSpec=z["userSpec"])
    assert np.array_equal(a, b)
    from scipy.interpolate import interp1d
    us = z["userSpec"][perm]
    fC = interp1d(np.log10(us[:, 0]), np.log10(us[:, 1]), kind="linear")
    inside = (f >= us[:, 0].min()) & (f <= us[:, 0].max())
    hc = 10.0 ** fC(np.log10(f[inside]))
    assert np.max(np.abs(a[inside] / (1 / 96 / np.pi ** 2 * hc ** 2 / f[inside] ** 3 * 3e8 * 10) - 1)) < 1e-12


def test_ra_dec_without_location_matches_the_reference_branches():
    """red_noise.py:203-221 leaves a pulsar without RAJ/DECJ/ELONG/ELAT at (0, 0); deterministic.py:76-91 fails on it."""
    from pta_replicator_amd._position import ra_dec

    class P:
        name, loc = "J0", {}
    assert ra_dec(P(), default=(0.0, 0.0)) == (0.0, 0.0)
    with pytest.raises(AttributeError):
        ra_dec(P())


def test_cgw_parameters_reproduce_the_oracle_waveform_on_the_host():
    """the 18 scalars handed to pta_cgw, pushed through a NumPy twin of the kernel body, equal oracle cgw_dt."""
    from pta_replicator_amd.deterministic import cgw_parameters
    mjd = np.linspace(53000, 57000, 50)
    base = dict(gwtheta=1.1, gwphi=4.0, mc=3e9, dist=40.0, fgw=2.2e-8, phase0=1.3, psi=0.4, inc=1.0, tref=53000 * 86400)
    for kw in (dict(pdist=1.3), dict(pdist=0.9, evolve=False, phase_approx=True), dict(pdist=1.1, evolve=False), dict(psrTerm=False),
               dict(pphase=2.1)):
        par, _, _, _ = cgw_parameters(0.7, 2.2, **base, **kw)
        tref, w0, ph0, w053, fac1, fac2, fac3, i1, i2, c2p, s2p, fp, fc, pdt = par[:14]
        toas = mjd * 86400 - tref
        tp = toas - pdt
        mode = int(par[14])
        if mode == 0:
            om, omp = w0 * (1 - fac1 * toas) ** (-3 / 8), w0 * (1 - fac1 * tp) ** (-3 / 8)
            ph, php = ph0 + fac2 * (w053 - om ** (-5 / 3)), ph0 + fac2 * (w053 - omp ** (-5 / 3))
        elif mode == 1:
            om, omp = w0, par[16]
            ph, php = ph0 + om * toas, par[17] + omp * toas
        else:
            om = omp = w0
            ph, php = ph0 + om * toas, ph0 + om * tp
        At, Bt, Atp, Btp = np.sin(2 * ph) * i1, np.cos(2 * ph) * i2, np.sin(2 * php) * i1, np.cos(2 * php) * i2
        al, alp = fac3 / om ** (1 / 3), fac3 / omp ** (1 / 3)
        rp, rc = al * (At * c2p + Bt * s2p), al * (-At * s2p + Bt * c2p)
        rpp, rcp = alp * (Atp * c2p + Btp * s2p), alp * (-Atp * s2p + Btp * c2p)
        res = fp * (rpp - rp) + fc * (rcp - rc) if par[15] else -fp * rp - fc * rc
        ref = po.cgw_dt(mjd, 0.7, 2.2, **base, **kw)
        assert np.max(np.abs(res - ref)) <= 1e-15 * np.max(np.abs(ref))


def test_array_pulsar_bookkeeping():
    from pta_replicator_amd._compat import TimeDelta, u
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    toas = ArrayTOAs(np.array([53000.0, 53010.0, 53020.0]), [0.5, 1.0, 2.0], [{"f": "a"}, {"f": "b"}, {"f": "a"}])
    psr = SimulatedPulsar(toas=toas, name="J0000+0000", loc={"RAJ": 1.0, "DECJ": 2.0})
    with pytest.raises(ValueError, match="make_ideal"):
        psr.update_added_signals("x", {})
    make_ideal(psr)
    dt = np.array([1e-6, -2e-6, 3e-6]) * u.s
    psr.update_added_signals("J0000+0000_x", {"p": 1}, dt)
    with pytest.raises(ValueError, match="already exists"):
        psr.update_added_signals("J0000+0000_x", {})
    psr.toas.adjust_TOAs(TimeDelta(dt.to("day")))
    psr.update_residuals()
    w = 1 / np.array([0.5, 1.0, 2.0]) ** 2
    expect = dt.value - np.sum(dt.value * w) / np.sum(w)
    assert np.max(np.abs(psr.residuals.resids_value - expect)) < 2e-12   # longdouble MJD resolution ~ 5e-12 s
    assert psr.toas.ntoas == 3 and psr.toas.get_errors().to("s").value[1] == 1.0 * 1e-6
    assert psr.toas.first_MJD.value == 53000.0 + float(np.longdouble(1e-6) / 86400) or abs(psr.toas.first_MJD.value - 53000.0) < 1e-9
    make_ideal(psr)
    assert np.all(psr.residuals.resids_value == 0) and psr.added_signals == {}


def test_par_tim_readers(tmp_path):
    from pta_replicator_amd.simulate import load_from_directories, load_pulsar, read_par_location
    par = tmp_path / "par"; tim = tmp_path / "tim"; par.mkdir(); tim.mkdir()
    (par / "A.par").write_text("PSR  J1234+5678\nRAJ  12:34:56.7 1\nDECJ  -56:07:08.9 1\nF0 100 1\n")
    (par / "B.par").write_text("PSR  B1855+09\nELONG  286.86 1\nELAT  32.32 1\n")
    for nm in ("A", "B"):
        (tim / f"{nm}.tim").write_text("FORMAT 1\nMODE 1\n x 1440.0 53000.000000000123 0.5 AXIS -f L-wide_ASP -be ASP\n"
                                       "C comment\n y 1440.0 53030.5 1.25 AXIS -f 430_PUPPI -pn -12.0\n")
    name, loc = read_par_location(str(par / "A.par"))
    assert name == "J1234+5678" and abs(loc["RAJ"] - (12 + 34 / 60 + 56.7 / 3600)) < 1e-12 and abs(loc["DECJ"] + (56 + 7 / 60 + 8.9 / 3600)) < 1e-12
    psrs = load_from_directories(str(par), str(tim))
    assert [p.name for p in psrs] == ["J1234+5678", "B1855+09"] and psrs[1].loc == {"ELONG": 286.86, "ELAT": 32.32}
    t = psrs[0].toas
    assert t.ntoas == 2 and t.flags[0] == {"f": "L-wide_ASP", "be": "ASP"} and t.flags[1]["f"] == "430_PUPPI"
    assert list(t.errors_us) == [0.5, 1.25] and float(t.mjd_ld[1]) == 53030.5
    with pytest.raises(FileNotFoundError):
        load_pulsar(str(par / "nope.par"), str(tim / "A.tim"))


def test_ecliptic_branch_restatement_is_sane():
    """ELONG/ELAT -> RA/DEC (PARITY UNPINNED: pyephem absent). Sanity: B1855+09 and J1909-3744 land on their
    catalogue positions to a few arcseconds."""
    from pta_replicator_amd._position import ecliptic_to_equatorial
    ra, dec = ecliptic_to_equatorial(284.2208542340, -15.1555138035, "J1909-3744")
    assert abs(np.degrees(ra) / 15 - (19 + 9 / 60 + 47.4 / 3600)) < 1e-3 and abs(np.degrees(dec) + (37 + 44 / 60 + 14.5 / 3600)) < 2e-3
    ra, dec = ecliptic_to_equatorial(286.863485782621126, 32.321482985635249, "B1855+09")  # B name -> epoch 1950
    assert abs(np.degrees(ra) / 15 - (18 + 55 / 60 + 13.7 / 3600)) < 2e-3 and abs(np.degrees(dec) - (9 + 39 / 60 + 13 / 3600)) < 5e-3


def test_ecliptic_branch_against_an_independent_evaluation_and_warns_once():
    """the libastro restatement (obliquity of the coordinate's epoch, two-leg IAU 1976 precession in rounded degrees) against an
    independent rotation-matrix evaluation with the arcsecond-valued IAU constants: agreement below a milliarcsecond bounds formula
    errors (the 7-decimal degree coefficients and the 84381.44796" obliquity differ from the IAU values at the 1e-10 rad level - the
    reason the ELONG / ELAT branch cannot be claimed at 1e-10 without a pyephem fixture); ra_dec() warns once per process."""
    import warnings
    from pta_replicator_amd import _position as pos
    asec = np.pi / 180 / 3600

    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        return {1: np.array([[1, 0, 0], [0, c, s], [0, -s, c]]), 2: np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]]),
                3: np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])}[axis]

    def independent(lon, lat, b1950):
        lam, bet = np.radians(lon), np.radians(lat)
        v = np.array([np.cos(bet) * np.cos(lam), np.cos(bet) * np.sin(lam), np.sin(bet)])
        v = rot(1, -84381.448 * asec) @ v                       # ecliptic -> equatorial, J2000
        if b1950:
            T = -0.5
            zeta, z, th = [(a * T + b * T ** 2 + c * T ** 3) * asec for a, b, c in
                           ((2306.2181, 0.30188, 0.017998), (2306.2181, 1.09468, 0.018203), (2004.3109, -0.42665, -0.041833))]
            v = rot(3, -z) @ rot(2, th) @ rot(3, -zeta) @ v      # IAU 1976 precession matrix J2000 -> date
        return np.arctan2(v[1], v[0]) % (2 * np.pi), np.arcsin(v[2])

    rng = np.random.default_rng(3)
    for lon, lat in [(286.863485782621126, 32.321482985635249), (284.2208542340, -15.1555138035)] + [(rng.uniform(0, 360), rng.uniform(-85, 85)) for _ in range(40)]:
        for name in ("B1855+09", "J1909-3744"):
            ra, dec = pos.ecliptic_to_equatorial(lon, lat, name)
            ra0, dec0 = independent(lon, lat, "B" in name)
            d = np.hypot((((ra - ra0) + np.pi) % (2 * np.pi) - np.pi) * np.cos(dec0), dec - dec0)
            assert d < 1e-3 * asec, (lon, lat, name, d / asec)

    class P:
        name = "B1855+09"
        loc = {"ELONG": 286.863485782621126, "ELAT": 32.321482985635249}
    if pos._ephem is None:
        pos._warned = False
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            pos.ra_dec(P)
            pos.ra_dec(P)
        assert len(w) == 1 and "1e-10" in str(w[0].message)


def test_population_split_matches_the_reference_bookkeeping():
    """deterministic.py:617-676 on the host: strain of every binary, loudest-per-bin selection (incl. an exact tie and a bin
    with fewer members than outlier_per_bin), free spectrum of the rest - against the reference run on the holodeck stub."""
    from pta_replicator_amd.deterministic import split_population
    z = load("population.npz")
    fc, free, hs, fo, mc, dl = split_population(z["vals"], z["weights"], z["fobs"], float(z["T_obs"]), outlier_per_bin=4)
    assert np.array_equal(fc, z["ret_f_centers"])
    assert np.max(np.abs(free / z["ret_free_spec"] - 1)) < 1e-13 and free[-1] == 1e-100
    assert hs.shape == (24,) and np.count_nonzero(hs) == 22
    assert np.array_equal(fo[fo > 0], z["ret_outlier_fo"])
    for got, key in ((hs, "outlier_hs"), (mc, "outlier_mc"), (dl, "outlier_dl")):
        assert np.max(np.abs(got[got > 0] / z["ret_" + key] - 1)) < 1e-13, key


def test_population_helpers_against_closed_forms():
    from pta_replicator_amd import _population as pop
    z = np.array([0.0, 1e-3, 0.5, 3.0, 12.0])
    try:
        om = pop.OMEGA_M
        pop.OMEGA_M = 1.0          # Einstein-de Sitter: d_c = 2c/H0 (1 - 1/sqrt(1+z))
        eds = 2 * pop.C_CGS * 1e-5 / pop.H0_KM_S_MPC * (1 - 1 / np.sqrt(1 + z)) * pop.PC_CGS * 1e6
        assert np.allclose(pop.comoving_distance_cm(z), eds, rtol=1e-12, atol=0)
    finally:
        pop.OMEGA_M = om
    assert abs(pop.comoving_distance_cm(1.0)[0] / (pop.PC_CGS * 1e6) - 3363.39) < 0.01     # WMAP9, no radiation
    m1, m2 = pop.component_masses(3.0, 0.5)
    assert (m1, m2) == (2.0, 1.0) and abs(pop.chirp_mass(m1, m2) - 2 ** 0.6 / 3 ** 0.2) < 1e-15
    # h_s of a 1e9 Msun chirp mass at 100 Mpc, f_gw = 2 f_orb = 1e-8 Hz: 8/sqrt(10) (G Mc)^(5/3) (pi f_gw)^(2/3) / (c^4 d)
    mcg, d, fgw = 1e9 * pop.MSOL_CGS, 100e6 * pop.PC_CGS, 1e-8
    expect = 8 / np.sqrt(10) * (pop.G_CGS * mcg) ** (5 / 3) * (np.pi * fgw) ** (2 / 3) / (pop.C_CGS ** 4 * d)
    assert abs(pop.gw_strain_source(mcg, d, fgw / 2) / expect - 1) < 1e-13


_BURST = dict(t0=2.2e8, tau=4.0e7, f=3.0e-8, a_plus=2.0e-7, a_cross=1.3e-7)      # as oracle/gen_golden.py


def _burst_plus(t, b=_BURST):
    return b["a_plus"] * np.exp(-0.5 * ((t - b["t0"]) / b["tau"]) ** 2) * np.cos(2 * np.pi * b["f"] * (t - b["t0"]))


def _burst_cross(t, b=_BURST):
    return b["a_cross"] * np.exp(-0.5 * ((t - b["t0"]) / b["tau"]) ** 2) * np.sin(2 * np.pi * b["f"] * (t - b["t0"]))


def test_burst_transient_and_memory_injectors_match_the_reference():
    """deterministic.py:718-884 - host-only by construction (user callables); golden from the unmodified reference."""
    from pta_replicator_amd.deterministic import add_burst, add_gw_memory, add_noise_transient
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    from helpers import relrms
    z = load("transients.npz")
    tref = 53000 * 86400

    def fresh():
        out = []
        for i in range(3):
            p = SimulatedPulsar(toas=ArrayTOAs(mjd_ld(z, "", i), z[f"err_us_{i}"]), name=str(z["names"][i]),
                                loc={"RAJ": float(z["raj_hours"][i]), "DECJ": float(z["decj_deg"][i])})
            make_ideal(p)
            out.append(p)
        return out

    def sig(p, key):
        return np.asarray(p.added_signals_time[f"{p.name}_{key}"].value, dtype=np.float64)

    for case, rq in (("burst", False), ("burst_quad", True)):
        for a, p in enumerate(fresh()):
            add_burst(p, 1.1, 4.0, _burst_plus, _burst_cross, psi=0.4, tref=tref, remove_quad=rq)
            assert relrms(sig(p, "burst"), z[case][a]) < 1e-12, (case, a)
    for a, p in enumerate(fresh()):
        add_noise_transient(p, _burst_plus, tref=tref)
        add_gw_memory(p, 3e-14, 0.7, 5.1, 0.9, 55500.0)
        assert relrms(sig(p, "noise_transient"), z["noise_transient"][a]) < 1e-12
        assert relrms(sig(p, "gw_memory"), z["gw_memory"][a]) < 1e-12
        with pytest.raises(ValueError):
            add_gw_memory(p, 3e-14, 0.7, 5.1, 0.9, 55500.0)          # same signal twice (simulate.py:85-86)


def test_array_enterprise_pulsar_hand_off(tmp_path):
    """to_enterprise() of an array-backed pulsar: enterprise's attribute surface, TOA-sorted, in enterprise's units; tim files
    written from a delay vector read back to the shifted TOAs."""
    from pta_replicator_amd.simulate import ArrayEnterprisePulsar, ArrayTOAs, SimulatedPulsar, make_ideal, read_tim
    from pta_replicator_amd._compat import TimeDelta, u
    rng = np.random.default_rng(4)
    mjd = rng.uniform(53000, 54000, 50)                     # unsorted on purpose
    flags = [{"f": "A" if i % 3 else "B", "pta": "NG"} for i in range(50)]
    psr = SimulatedPulsar(toas=ArrayTOAs(mjd, rng.uniform(0.2, 1.0, 50), flags=flags), name="J1234+5678", loc={"RAJ": 6.0, "DECJ": 30.0})
    make_ideal(psr)
    dt = rng.standard_normal(50) * 1e-6
    psr.update_added_signals("J1234+5678_test", {}, dt * u.s)
    psr.toas.adjust_TOAs(TimeDelta((dt * u.s).to("day")))
    psr.update_residuals()
    ep = psr.to_enterprise()
    assert isinstance(ep, ArrayEnterprisePulsar) and ep.name == "J1234+5678"
    order = np.argsort(mjd, kind="mergesort")
    assert np.all(np.diff(ep.toas) >= 0) and np.allclose(ep.toas, mjd[order] * 86400.0)
    assert np.allclose(ep.residuals, psr.residuals.resids_value[order], rtol=0, atol=1e-18)
    assert np.allclose(ep.toaerrs, psr.toas.errors_us[order] * 1e-6) and list(ep.backend_flags) == [flags[i]["f"] for i in order]
    assert ep.Mmat.shape == (50, 3) and np.linalg.matrix_rank(ep.Mmat) == 3
    assert abs(np.linalg.norm(ep.pos) - 1) < 1e-15 and abs(ep.theta - (np.pi / 2 - np.pi / 6)) < 1e-15 and abs(ep.phi - np.pi / 2) < 1e-15


def test_cw_source_params_is_bit_identical_to_the_per_source_scalar_loop():
    """one code path for every catalogue size.  The vectorised evaluation (array ufuncs + libm pow through
    pta_pow_host + np.dot's association through pta_dot3_host) must reproduce, BIT FOR BIT, the per-source loop on NumPy float64
    scalars that the reference's numba loop bodies run (deterministic.py:331-383) - here restated one source at a time."""
    from pta_replicator_amd import deterministic as det
    from pta_replicator_amd.constants import KPC2S, MPC2S, SOLAR2S
    rng = np.random.default_rng(11)
    n = 3000
    lists = [np.arccos(rng.uniform(-1, 1, n)), rng.uniform(0, 2 * np.pi, n), 10 ** rng.uniform(8, 10, n), 10 ** rng.uniform(1, 3, n),
             10 ** rng.uniform(-9, -7, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, np.pi, n), np.arccos(rng.uniform(-1, 1, n))]
    phat = np.array([0.3, -0.5, np.sqrt(1 - 0.34)])

    def loop(pdist, pphase):
        gwtheta, gwphi, mc, dist, fgw, phase0, psi, inc = lists
        par = np.zeros((n, det.CW_NPAR))
        for i in range(n):
            mci, di = mc[i] * SOLAR2S, dist[i] * MPC2S
            w0 = np.pi * fgw[i]
            w053 = w0 ** (-5 / 3)
            cgt, cgp, sgt, sgp = np.cos(gwtheta[i]), np.cos(gwphi[i]), np.sin(gwtheta[i]), np.sin(gwphi[i])
            m = np.array([sgp, -cgp, 0.0])
            nn = np.array([-cgt * cgp, -cgt * sgp, sgt])
            om = np.array([-sgt * cgp, -sgt * sgp, -cgt])
            fac1 = 256 / 5 * mci ** (5 / 3) * w0 ** (8 / 3)
            fac2 = 1 / 32 / mci ** (5 / 3)
            fac3 = mci ** (5 / 3) / di
            fplus = 0.5 * (np.dot(m, phat) ** 2 - np.dot(nn, phat) ** 2) / (1 + np.dot(om, phat))
            fcross = (np.dot(m, phat) * np.dot(nn, phat)) / (1 + np.dot(om, phat))
            cosMu = -np.dot(om, phat)
            pd = pphase / (2 * np.pi * fgw[i] * (1 - cosMu)) / KPC2S if pphase is not None else pdist
            pd = pd * KPC2S
            omega_p = w0 * (1 + fac1 * pd * (1 - cosMu)) ** (-3 / 8)
            par[i] = (w0, phase0[i] / 2, w053, fac1, fac2, fac3, 0.5 * (3 + np.cos(2 * inc[i])), 2 * np.cos(inc[i]), np.cos(2 * psi[i]),
                      np.sin(2 * psi[i]), fplus, fcross, pd * (1 - cosMu), omega_p, phase0[i] / 2 + fac2 * (w053 - omega_p ** (-5 / 3)), 0.0)
        return par

    for pdist, pphase in ((1.0, None), (0.7, None), (1.0, 1.3)):
        assert np.array_equal(loop(pdist, pphase), det.cw_source_params(lists, phat, pdist, pphase)), (pdist, pphase)
    assert det.cw_source_params([np.zeros(0)] * 8, phat).shape == (0, det.CW_NPAR)


def test_write_partim_round_trip_for_array_backed_pulsars(tmp_path):
    """simulate.py:71-77 for array-backed pulsars: the tim file carries the SHIFTED TOAs at longdouble precision, the par file is the
    one the pulsar was loaded from, verbatim (injection never changes the timing model); a pulsar built in code writes a minimal par
    (name + position) that the par reader parses back; the idealised design matrices have full column rank."""
    from pta_replicator_amd._compat import TimeDelta, u
    from pta_replicator_amd.simulate import (ArrayTOAs, SimulatedPulsar, load_pulsar, make_ideal, read_par_location, read_tim,
                                             timing_design_matrix)
    par_src = "PSR  J1234+5678\nRAJ  12:34:56.7 1\nDECJ  -56:07:08.9 1\nF0 100.123456789 1\nPEPOCH 55000\nDM 12.5\n"
    (tmp_path / "a.par").write_text(par_src)
    rng = np.random.default_rng(3)
    lines = ["FORMAT 1"] + [f" x 1440.0 {53000 + 7.3 * i:.13f} {0.5 + 0.01 * i:.3f} AXIS -f {'A' if i % 2 else 'B'} -be ASP" for i in range(40)]
    (tmp_path / "a.tim").write_text("\n".join(lines) + "\n")
    psr = load_pulsar(str(tmp_path / "a.par"), str(tmp_path / "a.tim"))
    make_ideal(psr)
    dt = rng.standard_normal(40) * 3e-6
    psr.update_added_signals("J1234+5678_x", {}, dt * u.s)
    psr.toas.adjust_TOAs(TimeDelta((dt * u.s).to("day")))
    psr.update_residuals()
    psr.write_partim(str(tmp_path / "out.par"), str(tmp_path / "out.tim"))
    assert (tmp_path / "out.par").read_text() == par_src
    mjd, err, freq, flags = read_tim(str(tmp_path / "out.tim"))
    assert np.max(np.abs((mjd - psr.toas.mjd_ld).astype(np.float64))) * 86400 < 1e-9          # < 1 ns through the text round trip
    assert np.max(np.abs((mjd - psr.toas.mjd0_ld).astype(np.float64) * 86400 - dt)) < 1e-9
    assert flags[1] == {"f": "A", "be": "ASP"} and np.allclose(err, psr.toas.errors_us)
    for loc in ({"RAJ": 18.961234, "DECJ": -9.72123}, {"ELONG": 286.86, "ELAT": 32.32}):
        q = SimulatedPulsar(toas=ArrayTOAs([53000.0, 53001.0], 1.0), name="J0000+0000", loc=loc)
        make_ideal(q)
        q.write_partim(str(tmp_path / "q.par"), str(tmp_path / "q.tim"))
        name, back = read_par_location(str(tmp_path / "q.par"))
        assert name == "J0000+0000" and set(back) == set(loc) and all(abs(back[k] - loc[k]) < 1e-9 for k in loc)
    t = np.sort(rng.uniform(53000, 58000, 400)) * 86400.0
    for model, m in (("spin", 3), ("astrometric", 9)):
        M, names = timing_design_matrix(t, model=model)
        assert M.shape == (400, m) and len(names) == m and np.linalg.matrix_rank(M) == m and np.max(np.abs(M)) <= 1.0 + 1e-12
    with pytest.raises(ValueError):
        timing_design_matrix(t, model="binary")


def test_native_legacy_normal_stream_equals_numpy_value_for_value():
    """pta_legacy_randn restates NumPy's legacy generator (MT19937 by init_genrand, 53-bit doubles, polar
    method with the cached second deviate): every deviate bit-identical to RandomState(seed).randn, for seeds at both ends of the
    32-bit range, odd counts (the cached deviate is carried from one randn call into the next), empty draws - and the GLOBAL stream
    is left exactly where the reference's sequential np.random.seed / randn calls (white_noise.py:79-80,105-109,154-155,182;
    red_noise.py:112-113,127,238-240) would leave it."""
    from pta_replicator_amd.white_noise import _legacy_normals
    seeds = [0, 1, 12345, 2 ** 32 - 1, 987654321, np.int64(77)]
    counts = [[7, 3], [1], [5000, 5001], [0, 2], [101], [3, 3, 3]]
    z = _legacy_normals(seeds, counts)
    after = np.random.randn(5)
    for sd, cs, zz in zip(seeds, counts, z):
        rs = np.random.RandomState(int(sd))
        for c, arr in zip(cs, zz):
            assert np.array_equal(rs.randn(c), arr), (sd, c)
    assert np.array_equal(after, rs.randn(5))            # the global stream continues from the last pulsar's state
    # seeds NumPy accepts but the native path does not (a sequence): RandomState path, same contract
    z2 = _legacy_normals([[1, 2, 3], 5], [[4], [4]])
    assert np.array_equal(z2[0][0], np.random.RandomState([1, 2, 3]).randn(4)) and np.array_equal(z2[1][0], np.random.RandomState(5).randn(4))
    np.random.seed(3)
    z3 = _legacy_normals(None, [[2000, 2001], [1500]])   # seed=None: ONE stream through the pulsars in order
    t3 = np.random.randn(3)
    np.random.seed(3)
    r3 = [[np.random.randn(2000), np.random.randn(2001)], [np.random.randn(1500)]]
    assert all(np.array_equal(a, b) for zz, rr in zip(z3, r3) for a, b in zip(zz, rr)) and np.array_equal(t3, np.random.randn(3))
    # thread count does not matter
    from pta_replicator_amd import _lib
    n = 9
    tot = np.full(n, 777, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(tot)]).astype(np.int64)
    sd = np.arange(100, 100 + n, dtype=np.uint32)
    outs = []
    for nt in (1, 3, 16):
        flat = np.empty(int(off[-1]))
        _lib.call("pta_legacy_randn", sd.ctypes.data, tot.ctypes.data, off.ctypes.data, n, flat.ctypes.data, None, None, None, nt)
        outs.append(flat)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0][:777], np.random.RandomState(100).randn(777))


def test_array_toas_float64_view_follows_the_toa_state():
    """ArrayTOAs caches the float64 rounding of its longdouble MJDs per TOA state: every accessor sees adjust_TOAs / reset_ideal,
    first_MJD / last_MJD equal the rounded longdouble extremes, and what get_mjds hands out is the caller's to modify."""
    from pta_replicator_amd.simulate import ArrayTOAs
    from pta_replicator_amd._compat import TimeDelta, u
    rng = np.random.default_rng(4)
    mjd = rng.uniform(53000, 58000, 257)
    t = ArrayTOAs(mjd, 0.5)
    m0 = t.get_mjds().value
    assert np.array_equal(m0, t.mjd_ld.astype(np.float64)) and t.first_MJD.value == float(t.mjd_ld.min()) and t.last_MJD.value == float(t.mjd_ld.max())
    m0 *= 0.0                                             # the caller's copy
    assert np.array_equal(t.get_mjds().value, t.mjd_ld.astype(np.float64))
    t.adjust_TOAs(TimeDelta((rng.uniform(-40, 40, 257)) * u.day))
    assert np.array_equal(t.get_mjds().value, t.mjd_ld.astype(np.float64))
    assert t.first_MJD.value == float(t.mjd_ld.min()) and t.last_MJD.value == float(t.mjd_ld.max())
    t.reset_ideal()
    assert np.array_equal(t.get_mjds().value, mjd) and t.first_MJD.value == mjd.min()


def test_ragged_cholesky_plan_is_end_aligned_and_sorted():
    """pta_potrf_ragged_plan (host code, no GPU): matrices sorted by decreasing order and dealt to the chains in turn; per chain the
    virtual order E = NB (T_max + 1) of its largest matrix, per matrix front = E - n and a virtual offset such that virtual element
    (front, front) is the matrix's own (0, 0); workspace = NB^2 doubles per matrix; odd orders / offsets / leading dimensions and
    unsupported flags are refused."""
    import ctypes
    from pta_replicator_amd import _lib
    n = np.array([300, 5000, 35038, 1024, 2050, 1026], dtype=np.int32)
    ld = ((n + 15) // 16 * 16).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n.astype(np.int64) * ld)])[:-1].astype(np.int64)
    B = len(n)

    def plan_for(flags):
        plan = np.zeros(int(_lib.lib.pta_potrf_ragged_plan_words(B)), dtype=np.int64)
        need = ctypes.c_int64(0)
        _lib.call("pta_potrf_ragged_plan", n.ctypes.data, off.ctypes.data, ld.ctypes.data, B, flags, plan.ctypes.data, ctypes.byref(need))
        return plan, need.value

    # (the default panel is 2048 columns here: the flop-weighted mean order of these six matrices is 35 000; 1024 below 16 384 - and
    # for fewer than six matrices whatever their orders: round 6, BASELINE config 2's three matrices)
    n3 = np.array([7758, 23024, 35038], dtype=np.int32)
    ld3 = ((n3 + 15) // 16 * 16).astype(np.int64)
    off3 = np.concatenate([[0], np.cumsum(n3.astype(np.int64) * ld3)])[:-1].astype(np.int64)
    plan3 = np.zeros(int(_lib.lib.pta_potrf_ragged_plan_words(3)), dtype=np.int64)
    _lib.call("pta_potrf_ragged_plan", n3.ctypes.data, off3.ctypes.data, ld3.ctypes.data, 3, 0, plan3.ctypes.data, ctypes.byref(ctypes.c_int64(0)))
    assert plan3[4] == 1024 and plan3[3] == 2
    for flags, nchain, NB in ((0, 2, 2048), (_lib.POTRF_CHAINS(3) | _lib.POTRF_NB(1), 3, 256), (_lib.POTRF_NO_LOOKAHEAD | _lib.POTRF_NB(4), 1, 1024)):
        plan, need = plan_for(flags)
        assert plan[1] == B and plan[3] == nchain and plan[4] == NB and plan[5] == need == B * NB * NB
        order = sorted(range(B), key=lambda b: (-n[b], b))
        seen = []
        for c in range(nchain):
            h = plan[8 + 8 * c: 16 + 8 * c]
            Bc, E, Tmax, w0 = int(h[0]), int(h[1]), int(h[2]), int(h[3])
            idx = plan[w0 + 3 * Bc: w0 + 4 * Bc]
            assert list(idx) == order[c::nchain]                       # dealt in turn: every chain gets the same mix of orders
            nn = plan[w0 + 4 * Bc: w0 + 5 * Bc]
            assert list(nn) == [int(n[b]) for b in idx] and all(nn[k] >= nn[k + 1] for k in range(Bc - 1))
            assert Tmax == (nn[0] - 1) // NB and E == NB * (Tmax + 1)
            front = plan[w0 + 2 * Bc: w0 + 3 * Bc]
            assert list(front) == [E - int(x) for x in nn]
            offv, ldv = plan[w0: w0 + Bc], plan[w0 + Bc: w0 + 2 * Bc]
            for k, b in enumerate(idx):
                assert ldv[k] == ld[b] and offv[k] + front[k] * (ld[b] + 1) == off[b]      # virtual (front, front) = the matrix's (0, 0)
            seen += list(idx)
        assert sorted(seen) == list(range(B))
    for bad in (dict(n=np.array([101], dtype=np.int32)), dict(ld=np.array([111], dtype=np.int64)), dict(off=np.array([3], dtype=np.int64))):
        a = dict(n=np.array([100], dtype=np.int32), off=np.array([0], dtype=np.int64), ld=np.array([112], dtype=np.int64))
        a.update(bad)
        plan = np.zeros(int(_lib.lib.pta_potrf_ragged_plan_words(1)), dtype=np.int64)
        with pytest.raises(_lib.PtaError):
            _lib.call("pta_potrf_ragged_plan", a["n"].ctypes.data, a["off"].ctypes.data, a["ld"].ctypes.data, 1, 0, plan.ctypes.data, ctypes.byref(ctypes.c_int64(0)))
    # a tampered plan is refused before anything is launched (header and per-chain consistency checks; no GPU needed to see it)
    plan, need = plan_for(0)
    for word, value in ((0, 1), (3, 7), (4, 1000), (8, B + 1), (9, 12345)):
        bad = plan.copy()
        bad[word] = value
        rc = _lib.lib.pta_potrf_ragged(ctypes.c_void_p(16), bad.ctypes.data, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), need, None)
        assert rc == -1 and "plan" in _lib.last_error(), (word, rc, _lib.last_error())
    plan = np.zeros(int(_lib.lib.pta_potrf_ragged_plan_words(B)), dtype=np.int64)
    with pytest.raises(_lib.PtaError):   # the VALU / substitution cross-check paths have no ragged form
        _lib.call("pta_potrf_ragged_plan", n.ctypes.data, off.ctypes.data, ld.ctypes.data, B, _lib.POTRF_SUBSTITUTION, plan.ctypes.data, ctypes.byref(ctypes.c_int64(0)))


def test_bench_ragged_workload_definition():
    """bench.ragged_counts: the ng15-like spread of TOA counts the ragged TD figures are quoted on (42 quantiles of the log-uniform
    distribution on [500, 35000]: sum 340 915 = the headline array's total, 46.9 TFLOP of factorisation), shuffled but reproducible;
    bench.ragged_array builds pulsars of exactly those counts with the ng15 noise values cycled."""
    import bench
    c = bench.ragged_counts()
    assert len(c) == 42 and sum(c) == 340915 and min(c) == 526 and max(c) == 33274
    assert c == bench.ragged_counts() and c != sorted(c) and c != sorted(c, reverse=True)
    assert abs(sum(float(n) ** 3 for n in c) / 3 / 1e12 - 46.9146) < 1e-3
    psrs, noise = bench.ragged_array(c[:3])
    assert [p.toas.ntoas for p in psrs] == c[:3]
    assert len(noise["efac"]) == 3 and len(noise["flags"][0]) == len(noise["efac"][0])
    for p, fl in zip(psrs, noise["flags"]):
        assert {f["f"] for f in p.toas.flags} <= set(fl)


def test_native_pair_separations_equal_the_scalar_loop_bit_for_bit():
    """pair_zeta_cos (native arccos arguments + one NumPy arccos / cos over the pair array) against the per-pair scalar loop
    the reference runs (spharmORFbasis.py:14-35,400-408) - array_equal on all 20 100 pairs of BASELINE config 5's geometry, on a geometry
    with repeated positions (the exact-equality branch), near-antipodal and near-coincident pairs (arguments at and beyond +-1), and on
    small arrays (every pair re-derived by the self-check); the fallback switch hands the loop's numbers back unchanged."""
    import time
    from pta_replicator_amd import spharmORFbasis as anis
    rng = np.random.default_rng(200)
    P = 200
    raj, decj = rng.uniform(0, 24, P), np.degrees(np.arcsin(rng.uniform(-1, 1, P)))
    locs = np.ascontiguousarray(np.stack([raj * np.pi / 12.0, np.pi / 2.0 - np.radians(decj)], axis=1))
    t0 = time.perf_counter()
    ref = anis.pair_zeta_cos_loop(locs)
    t1 = time.perf_counter()
    got = anis.pair_zeta_cos(locs)
    t2 = time.perf_counter()
    assert anis._native_pairs_ok
    assert np.array_equal(ref, got)
    assert (t2 - t1) < 0.5 * (t1 - t0)                      # 61 ms -> ~1.5 ms here (the sampled self-check included)
    # repeated positions, antipodes, poles, nearly identical positions
    sp = np.array([[1.0, 0.7], [1.0, 0.7], [1.0 + np.pi, np.pi - 0.7], [0.3, 0.0], [2.9, np.pi], [1.0, 0.7 + 1e-9], [1.0 + 1e-15, 0.7],
                   [4.0, 1.5707963267948966], [4.0 - np.pi, 1.5707963267948966], [5.5, 1e-300]])
    ref = anis.pair_zeta_cos_loop(sp)
    got = anis.pair_zeta_cos(sp)
    assert np.array_equal(ref, got)
    assert got[0, 1, 0] == 0.0 and got[0, 1, 1] == 1.0 and abs(got[0, 2, 0] - np.pi) < 1e-7
    for seed in range(5):
        r2 = np.random.default_rng(seed)
        q = np.stack([r2.uniform(0, 2 * np.pi, 7), np.arccos(r2.uniform(-1, 1, 7))], axis=1)
        assert np.array_equal(anis.pair_zeta_cos_loop(q), anis.pair_zeta_cos(q))
    anis._native_pairs_ok = False
    try:
        assert np.array_equal(anis.pair_zeta_cos(sp), ref)
    finally:
        anis._native_pairs_ok = True


def test_enterprise_toas_have_one_error_column_and_edited_positions_win():
    """EnterpriseTOAs keeps ONE error column (the caller's seconds); errors_us is a view of it, so rescaling either is seen by
    get_errors(), errors_seconds() and write_tim alike.  loc['RA_RAD'] / ['DEC_RAD'] (the unrounded radians of an enterprise-style pulsar)
    are used only while they still agree with RAJ / DECJ: an edited RAJ / DECJ wins."""
    from pta_replicator_amd import simulate as sim, white_noise as wn
    from pta_replicator_amd._position import ra_dec
    t = sim.EnterpriseTOAs(np.arange(5) * 86400.0 + 4.6e9, np.array([1e-6, 2e-6, 3e-7, 4e-6, 5e-6]))
    e0 = wn.errors_seconds(t).copy()
    assert np.array_equal(e0, [1e-6, 2e-6, 3e-7, 4e-6, 5e-6]) and np.allclose(t.errors_us, e0 * 1e6, rtol=1e-15)
    t.errors_us = t.errors_us * 2.0                                   # a caller rescales the microsecond column
    assert np.allclose(wn.errors_seconds(t), 2 * e0, rtol=1e-15) and np.allclose(np.asarray(t.get_errors().to("s").value), 2 * e0, rtol=1e-15)
    t.errors_s = e0 * 3.0                                             # ... or the seconds
    assert np.allclose(t.errors_us, 3e6 * e0, rtol=1e-15) and np.allclose(wn.errors_seconds(t), 3 * e0, rtol=1e-15)

    class P:
        name = "J0000+0000"
        loc = {"RAJ": 1.0 * 12.0 / np.pi, "DECJ": np.degrees(0.5), "RA_RAD": 1.0, "DEC_RAD": 0.5}
    assert ra_dec(P) == (1.0, 0.5)
    P.loc = dict(P.loc, RAJ=6.0, DECJ=30.0)                           # edited afterwards: RAJ / DECJ are what the caller means
    ra, dec = ra_dec(P)
    assert abs(ra - np.pi / 2) < 1e-15 and abs(dec - np.pi / 6) < 1e-15


def test_td_strip_table_puts_the_partial_strip_first():
    """engine_td._strips (round 6): every factor's rows are tiled without gap or overlap by strips of <= 256 rows whose first rows are multiples of
    16; an order that is not a multiple of 256 has its PARTIAL strip first (K extent = its own height) and whole strips behind it, so that no
    strip with a long K extent carries dead column tiles (at most the < 16 rows that complete the last tile); items come longest K first."""
    from pta_replicator_amd.engine_td import _strips
    counts = [5000, 600, 256, 257, 255, 1, 16, 17, 512, 10000, 7758, 35037]
    blk, n0, rows = _strips(counts)
    assert len(blk) == len(n0) == len(rows)
    kext = [min(counts[b], s + r) for b, s, r in zip(blk, n0, rows)]
    assert kext == sorted(kext, reverse=True)
    for b, n in enumerate(counts):
        it = sorted((int(s), int(r)) for bb, s, r in zip(blk, n0, rows) if bb == b)
        assert it[0][0] == 0 and all(s % 16 == 0 and 1 <= r <= 256 for s, r in it)
        assert all(it[i][0] + it[i][1] == it[i + 1][0] for i in range(len(it) - 1)) and it[-1][0] + it[-1][1] == n
        assert len(it) == -(-n // 256)                                   # no more strips than before
        assert all(r == 256 for _, r in it[1:-1])
        if n % 256 and len(it) > 1:
            assert it[0][1] == min(256, (n % 256 + 15) // 16 * 16) and it[-1][1] > 256 - 16      # the last strip lacks less than one tile
    b5000 = sorted((int(s), int(r)) for bb, s, r in zip(blk, n0, rows) if bb == 0)
    assert b5000[0] == (0, 144) and b5000[-1] == (4752, 248)
    # matrix-pipe work of the launch ~ sum over strips of 256 x K extent: 3.9 % less at 5000 TOAs than with the partial strip last
    new = sum(256 * min(5000, s + r) for s, r in b5000)
    old = sum(256 * min(5000, k + 256) for k in range(0, 5000, 256))
    assert 0.958 < new / old < 0.964


def test_bench_line_roofline_fits_the_driver_record():
    """VERDICT r5 #1a: the driver's record keeps the first 24 keys of `roofline`, names cut at 40 characters, strings at 120 - two rounds of
    TD-mode fractions (BASELINE.json's "fp64 Cholesky MFMA util %" half of the metric) were cut off behind longer lists.  compact_line on a
    full record with EVERY source field present: <= 24 keys, every name <= 40 characters, the contract's eight first and in order, the TD
    fractions inside the kept prefix, no string over 120 characters anywhere in the two flat objects; the line stays one JSON line."""
    import json
    import bench
    long = "x" * 400
    full = {"metric": "realizations/sec, 68 psr x 5000 TOAs GWB+RN+WN", "value": 2.1e5, "unit": "realizations/s", "n_gpus": 1, "steps": 20, "warmup": 5,
            "ms_per_step": 4.86, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": long, "realisations_per_step_per_gpu": 1024},
            "roofline": {"kernel": "pta_engine_synth", "bound": "fp64-valu (rng)", "bound_by_contract_enum": "hbm", "achieved": 959.4, "peak": 8000.0, "unit": "GB/s",
                         "frac": 0.1199, "traffic": 3.36e9, "avg_launch_ms": 2.9, "engine_clock_GHz": 2.3,
                         "valu_issue": {"insts_valu_per_output_element": 219.3, "frac_of_launch_at_measured_clock": 0.7},
                         "also": {"kernel": "pta_gwb_czt", "stage_ms": 2.07, "frac": 0.51}},
            "step": {"frac_of_fp64_peak": 0.336, "normals_T_per_s": 0.296, "frac_of_rng_microbench": 0.49},
            "microbench": {"fp64_mfma_tile_tflops": 72.3, "hbm_write_TBps": 4.37, "normals_T_per_s": 0.6},
            "orf_config5": {"orf_basis_ms": 0.38, "orf_combine_ms": 0.005, "host_pair_separations_ms": 0.9, "host_pair_separations_python_loop_ms": 61.0},
            "td_mode": {"cov_assemble_kernel": "walk", "cov_assemble_ms": 2.05, "cov_assemble_GBps_lower_triangle": 3323.0, "cov_assemble_walk_ms": 2.05,
                        "cov_assemble_tile_ms": 2.95, "potrf_ms": 53.0, "potrf_TFLOPs": 53.4, "potrf_frac_of_fp64_mfma_peak": 0.68,
                        "potrf_trailing_update_mfma_busy_pct": 83.8, "generate_td_ms": 30.07, "trmm_useful_TFLOPs": 57.9, "trmm_frac_of_fp64_mfma_peak": 0.737,
                        "realisations_per_s": 34053.0, "prepare_td_first_call_ms": 244.3, "prepare_td_ms": 56.0,
                        "ragged": {"potrf_TFLOPs": 62.2, "potrf_frac_of_fp64_mfma_peak": 0.792, "trmm_frac_of_fp64_mfma_peak": 0.798, "cov_assemble_TBps": 3.4},
                        "config2_shape": {"potrf_frac_of_fp64_mfma_peak": 0.69, "realisations_per_s": 31500.0}},
            "cpu_baseline": {"value": 0.34, "unit": "realisations/s", "cores": 1, "kind": "port", "sample": long, "value_without_ecorr": 3.66, "host_cpus": 256,
                             "reference_container": {"value": 0.056, "value_without_ecorr": 0.71, "cores": 8, "date": "2026-09-30"}},
            "grid": [{"n_psr": 3, "n_toa": 122, "throughput": {"realisations_per_s": 7.7e6}, "td": {"potrf_frac": 0.0, "trmm_frac": 0.0},
                      "cpu": {"realisations_per_s": 55.0, "kind": "port", "cores": 1}}],
            "kernels_ms": {"pta_engine_synth": 2.9}}
    line = bench.compact_line(full)
    roof = line["roofline"]
    assert len(roof) <= 24 and bench.ROOFLINE_MAX_KEYS == 24
    assert all(len(k) <= 40 for k in roof), [k for k in roof if len(k) > 40]
    assert list(roof)[:8] == ["kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms"]
    for k in ("td_potrf_frac", "td_potrf_mfma_busy_pct", "td_trmm_frac", "td_cov_frac_hbm", "td_cov_TBps", "td_realisations_per_s", "td_ragged_potrf_frac",
              "td_prepare_first_call_ms", "step_frac_of_fp64_peak", "valu_insts_per_out_elem", "box_fp64_mfma_TFLOPs", "box_hbm_write_TBps",
              "orf_basis_ms_P200_lmax4", "frac_rng"):
        assert roof[k] is not None, k
    assert roof["bound"] == "fp64-valu (rng)" and roof["td_potrf_frac"] == 0.68 and roof["td_realisations_per_s"] == 34053.0
    assert abs(roof["td_cov_frac_hbm"] - 3323.0 / 8000.0) < 1e-4
    cpu = line["cpu_baseline"]
    assert len(cpu) <= 12 and all(len(k) <= 40 for k in cpu)
    assert cpu["reference_in_build_container"] == 0.056 and cpu["reference_date"] == "2026-09-30"
    for obj in (roof, cpu, line["config"]):
        assert all(len(v) <= 120 for v in obj.values() if isinstance(v, str))
    assert line["grid"][0]["cpu_real_per_s"] == 55.0 and line["grid"][0]["cpu_kind"] == "port"
    txt = json.dumps(line)
    assert "\n" not in txt and len(txt) < 8000
    # an empty record (N > 1 ranks carry no TD / microbench blocks) still yields the contract's keys
    empty = bench.compact_line({"roofline": {"kernel": "k", "bound": "hbm"}})
    assert list(empty["roofline"])[:8] == list(roof)[:8] and len(empty["roofline"]) <= 24


def test_bench_dump_outputs_is_a_bounded_seeded_sample(tmp_path):
    """bench.py --dump-outputs: a small batch is written whole; a large one as the same seeded sample of whole realisations on every
    run, within 64 MB, float64, with the realisation number of each row; a realisation too long for the budget is sampled by TOA too."""
    import os
    import torch
    import bench

    def dump(out, name):
        bench.dump_outputs(out, 40, str(tmp_path / name))
        files = sorted(os.listdir(tmp_path / name))
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64e6
        return {f[:-4]: np.load(tmp_path / name / f) for f in files}

    small = torch.arange(6 * 50, dtype=torch.float64).reshape(6, 50)
    z = dump(small, "small")
    assert set(z) == {"residuals", "realisation"} and np.array_equal(z["residuals"], small.numpy())
    assert np.array_equal(z["realisation"], np.arange(40, 46, dtype=np.float64))
    n = 340000                                       # the headline array's TOA count
    big = torch.arange(64, dtype=torch.float64)[:, None] * 1e6 + torch.arange(n, dtype=torch.float64)[None, :]
    a, b = dump(big, "big_a"), dump(big, "big_b")
    rows = a["realisation"].astype(int) - 40
    assert a["residuals"].dtype == np.float64 and len(rows) == bench.DUMP_MAX_BYTES // (8 * n) and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["residuals"], big.numpy()[rows]) and all(np.array_equal(a[k], b[k]) for k in a)
    long = torch.zeros((2, bench.DUMP_MAX_BYTES // 8 + 1), dtype=torch.float64)
    c = dump(long, "long")
    assert set(c) == {"residuals", "realisation", "toa_index"} and c["residuals"].shape == (1, len(c["toa_index"]))


def test_from_enterprise_adapter_reads_enterprise_style_arrays():
    """VERDICT r4 #6 / SURVEY.md §7 step 2: an object with enterprise's array surface (toas [s], toaerrs [s], flags dict, backend_flags,
    _raj/_decj or theta/phi or pos) becomes an array-backed SimulatedPulsar that the add_* functions and the engine take; the numbers the
    injection path reads come back bit for bit when the TOAs lie on a grid float64 holds exactly (x * 86400 / 86400)."""
    from pta_replicator_amd._position import ra_dec
    from pta_replicator_amd.simulate import (ArrayEnterprisePulsar, ArrayTOAs, SimulatedPulsar, as_simulated, from_enterprise, is_enterprise_like,
                                             make_ideal)
    rng = np.random.default_rng(8)
    mjd = np.sort(53000.0 + rng.integers(0, 3000 * 1024, 80) / 1024.0)      # multiples of 1/1024 day: the seconds <-> days round trip is exact
    flags = [{"f": "A" if i % 3 else "B", "pta": "NG"} if i % 5 else {"f": "A"} for i in range(80)]
    src = SimulatedPulsar(toas=ArrayTOAs(mjd, rng.uniform(0.2, 1.0, 80), flags=flags), name="J1234+5678", loc={"RAJ": 6.3, "DECJ": -31.7})
    make_ideal(src)
    ep = src.to_enterprise()
    assert isinstance(ep, ArrayEnterprisePulsar) and is_enterprise_like(ep) and not is_enterprise_like(src)
    assert as_simulated(src) is src
    psr = from_enterprise(ep)
    assert psr.name == "J1234+5678" and psr.added_signals == {} and psr.toas.ntoas == 80
    assert np.array_equal(psr.toas.get_mjds().value, src.toas.get_mjds().value)
    assert np.array_equal(np.array(psr.toas.table["tdbld"], dtype="float64") * 86400, np.array(src.toas.table["tdbld"], dtype="float64") * 86400)
    assert np.array_equal(psr.toas.get_errors().to("s").value, src.toas.get_errors().to("s").value)
    assert [f["f"] for f in psr.toas.table["flags"].data] == [f["f"] for f in flags]
    assert ["pta" in f for f in psr.toas.table["flags"].data] == ["pta" in f for f in flags]     # '' (flag absent) does not become a flag
    assert ra_dec(psr) == ra_dec(src)
    # position fall-backs: theta / phi, then the unit vector
    class Bare:
        pass
    b = Bare()
    b.name, b.toas, b.toaerrs, b.flags, b.backend_flags = "J0000+0000", ep.toas, ep.toaerrs, {}, ep.backend_flags
    b.theta, b.phi = ep.theta, ep.phi
    p2 = from_enterprise(b)
    assert np.allclose(ra_dec(p2), ra_dec(src), rtol=0, atol=1e-15) and [f["f"] for f in p2.toas.table["flags"].data] == list(ep.backend_flags)
    del b.theta, b.phi
    b.pos = ep.pos
    assert np.allclose(ra_dec(from_enterprise(b)), ra_dec(src), rtol=0, atol=1e-15)
    del b.pos
    with pytest.raises(AttributeError):
        from_enterprise(b)


def test_walk_assembly_item_table_matches_its_definition():
    """pta_td_cov_walk_items (host side of the column-walking TD assembly kernel): work items = (pulsar, 256-column group, 512-row segment of
    the rows from the group's first column down) - item0[b] = first item of pulsar b, item0[P] = total = what the launch's grid will be."""
    import ctypes
    from pta_replicator_amd import _lib
    rng = np.random.default_rng(3)
    for counts in ([5000] * 68, [1], [2, 255, 256, 257, 511, 512, 513, 1024, 35037], list(rng.integers(1, 40000, 42))):
        n = np.ascontiguousarray(counts, dtype=np.int32)
        item0 = np.zeros(len(n) + 1, dtype=np.int32)
        for variant in (0, 1):
            tot = _lib.lib.pta_td_cov_walk_items(ctypes.c_void_p(n.ctypes.data), len(n), 60, variant, ctypes.c_void_p(item0.ctypes.data))
            want = [sum(-(-(int(c) - 256 * cb) // 512) for cb in range(-(-int(c) // 256))) for c in counts]
            assert tot == sum(want) == item0[-1] and list(np.diff(item0)) == want
    assert _lib.lib.pta_td_cov_walk_items(None, 3, 60, 0, ctypes.c_void_p(item0.ctypes.data)) == -1
    assert _lib.lib.pta_td_cov_walk_items(ctypes.c_void_p(n.ctypes.data), len(n), 60, 7, ctypes.c_void_p(item0.ctypes.data)) == -1
