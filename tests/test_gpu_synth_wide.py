"""The fused synthesis kernel with two pairs of ADJACENT TOAs per lane (16-byte loads of the design matrix, 16-byte stores of the result
rows: synth_variant 0 and the hooks 16 / 48) against the kernel as it was (synth_variant 2: a lane's TOAs 16 apart, 8-byte accesses).
Every dot product sums the same K-steps in the same order and every draw has the same counter - the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# TOAs per pulsar: a tile of one TOA (that pulsar has no red noise), fewer than four, one short of a full tile (the 8-byte path up to
# its last lane), exactly one tile, one / four past it (a short tile of one wave, the other three retire early), two full tiles and three TOAs
COUNTS = (1, 3, 255, 256, 257, 260, 515)
RS = (1, 5, 16, 17, 33)     # realisation rows: below, at and past one / two groups of 16
R0 = 11


@pytest.fixture(scope="module")
def psrs():
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(1717)
    out = []
    for a, n in enumerate(COUNTS):
        # observing epochs of three TOAs each, minutes apart: several TOAs share an ECORR epoch, and epochs straddle tile boundaries
        ep = np.sort(rng.uniform(53000, 57500, (n + 2) // 3))
        mjd = np.sort((np.repeat(ep, 3)[:n] + rng.uniform(0, 0.01, n)))
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, 0.5), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


def _engine(psrs, components, without=None):
    from pta_replicator_amd.engine import ReplicaEngine
    P = len(COUNTS)
    eng = ReplicaEngine(psrs, seed=9091)
    eng.td_warmup = False
    lA = [None] + list(np.linspace(-14.3, -13.4, P - 1))   # the one-TOA pulsar carries no red noise
    eng.set_red_noise(lA, [None] + list(np.linspace(2.2, 4.4, P - 1)), components=components)
    if without != "wn":
        eng.set_white_noise(efac=list(np.linspace(0.8, 1.4, P)), log10_equad=list(np.linspace(-6.9, -6.1, P)))
    if without != "ecorr":
        eng.set_jitter(log10_ecorr=list(np.linspace(-6.8, -6.2, P)), coarsegrain=0.1)
    if without != "gwb":
        eng.set_gwb(-14.2, 13. / 3.)
    eng.prepare()
    assert eng.K == 2 * components
    return eng


# components 30 / 29 / 1: K = 60 (the headline's), 58 and 2 - the last two leave a partial group of four bins
@pytest.mark.parametrize("components", [30, 29, 1])
@pytest.mark.parametrize("without", [None, "gwb", "wn", "ecorr"])
def test_adjacent_toas_bit_identical(psrs, components, without):
    import torch
    eng = _engine(psrs, components, without)
    if without != "ecorr":   # epochs are shared, and staged through LDS
        assert all(len(np.unique(e)) < len(e) for e, n in zip(eng.epoch_of, COUNTS) if n >= 3)
    for R in RS:
        eng.synth_variant = 2
        ref = eng.generate(R, r0=R0).clone()
        assert ref.shape == (R, sum(COUNTS)) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        for variant in (0, 16, 48):   # default; scalar row offsets with the complete-plan copy where complete; with the copy for any plan
            eng.synth_variant = variant
            got = eng.generate(R, r0=R0)
            assert torch.equal(got, ref), (components, without, R, variant)


def test_rows_eight_byte_aligned(psrs):
    """out as a view of a wider buffer that starts at an odd column, odd leading dimension: every row is 8-byte, no row 16-byte
    aligned throughout - and nothing outside the view is written."""
    import torch
    from pta_replicator_amd import device as dv
    eng = _engine(psrs, 30)
    n = eng.n_toa
    for R in RS:
        bufs = {}
        for variant in (2, 0, 16, 48):
            big = dv.empty((R, n + 6))
            big.fill_(float("nan"))
            view = big[:, 3:3 + n]
            assert view.stride(0) == n + 6 and view.data_ptr() % 16 == 8
            eng.synth_variant = variant
            eng.generate(R, r0=R0, out=view)
            bufs[variant] = big
        ref = bufs[2]
        assert bool(torch.isfinite(ref[:, 3:3 + n]).all())
        assert bool(torch.isnan(ref[:, :3]).all()) and bool(torch.isnan(ref[:, 3 + n:]).all())
        for variant in (0, 16, 48):
            assert torch.equal(bufs[variant][:, 3:3 + n], ref[:, 3:3 + n]), (R, variant)
            assert bool(torch.isnan(bufs[variant][:, :3]).all()) and bool(torch.isnan(bufs[variant][:, 3 + n:]).all()), (R, variant)


@pytest.mark.parametrize("components", [29, 30])
def test_engine_against_the_oracle_on_host_only_draws(psrs, components):
    """prepare()'s tables, the kernel and the Philox twin tied together at these shapes with no device-drawn number in the reference:
    the draws of realisations 2^32 - 3 ... from oracle/philox_ref.py alone equal the dumped ones (to the bound of
    test_rng_fill_matches_numpy_twin), and generate() agrees with the CPU oracle evaluated on them, per pulsar."""
    from helpers import host_draws, relrms
    from oracle import pta_oracle as po
    eng = _engine(psrs, components)
    P, R, r0 = len(COUNTS), 17, 2 ** 32 - 3
    lA, gam = [None] + list(np.linspace(-14.3, -13.4, P - 1)), [None] + list(np.linspace(2.2, 4.4, P - 1))
    efac, leq, lec = np.linspace(0.8, 1.4, P), np.linspace(-6.9, -6.1, P), np.linspace(-6.8, -6.2, P)
    grid = po.gwb_grid([float(m.min()) for m in eng.mjd], [float(m.max()) for m in eng.mjd])
    Mchol = np.linalg.cholesky(po.hd_orf_closed_form(po.psr_locs_equatorial([p.loc for p in psrs])))
    C = po.gwb_spectrum(grid["f"], grid["dur"], grid["howml"], -14.2, 13. / 3.)
    quant = [po.quantize(eng.mjd[a], dt=0.1) for a in range(P)]
    out = eng.generate(R, r0=r0).cpu().numpy()
    assert out.shape == (R, sum(COUNTS)) and np.all(np.isfinite(out))
    for r in range(R):
        d, dev = host_draws(eng, r0 + r), eng.dump_draws(r0 + r)
        assert d.keys() == dev.keys() == {"gwb", "rn", "wn", "ecorr"}
        assert d["gwb"].shape == dev["gwb"].shape and np.max(np.abs(d["gwb"] - dev["gwb"])) < 1e-13
        for a in range(P):
            assert d["rn"][a].shape == dev["rn"][a].shape and np.max(np.abs(d["rn"][a] - dev["rn"][a])) < 1e-13
            assert d["ecorr"][a].shape == dev["ecorr"][a].shape and np.max(np.abs(d["ecorr"][a] - dev["ecorr"][a])) < 1e-13
            for k in range(2):
                assert d["wn"][a][k].shape == dev["wn"][a][k].shape and np.max(np.abs(d["wn"][a][k] - dev["wn"][a][k])) < 1e-13
        res_gw, _ = po.gwb_dt(grid, Mchol, d["gwb"], C, [m * 86400 for m in eng.mjd])
        for a in range(P):
            n = COUNTS[a]
            ref = po.measurement_noise_dt(eng.sigma_s[a], np.ones(n) * efac[a], np.ones(n) * 10 ** leq[a], *d["wn"][a])
            epoch_of, ne, first, _ = quant[a]
            ref = ref + po.jitter_dt(epoch_of, po.jitter_ecorr_vector(ne, first, lec[a]), d["ecorr"][a]) + res_gw[a]
            if lA[a] is not None:
                ref = ref + po.red_noise_dt(psrs[a].toas.table["tdbld"], lA[a], gam[a], d["rn"][a], components=components)
            assert relrms(out[r, eng.off[a]:eng.off[a + 1]], ref) < 1e-10, (components, r, a)
