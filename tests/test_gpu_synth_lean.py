"""The fused synthesis kernel's red-noise loop with scalar row offsets (synth_variant 0) against the per-lane 64-bit index products
(synth_variant 2): the same loads, the same MFMA sequence - the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (300, 256, 17)   # one full + one partial tile, exactly one full tile, a pulsar shorter than a wave


@pytest.fixture(scope="module")
def psrs():
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(21)
    out = []
    for a, n in enumerate(COUNTS):
        mjd = np.sort(rng.uniform(53000, 57500, n))
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, 0.5), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


# components 30 / 7 / 1: K = 60 (the headline's), 14 and 2 - the last two leave a partial group of four bins
@pytest.mark.parametrize("components", [30, 7, 1])
@pytest.mark.parametrize("everything", [True, False])
def test_scalar_row_offsets_bit_identical(psrs, components, everything):
    import torch
    from pta_replicator_amd.engine import ReplicaEngine
    P = len(COUNTS)
    eng = ReplicaEngine(psrs, seed=4321)
    eng.td_warmup = False
    eng.set_red_noise([-13.8, -14.2, -13.5], [3.1, 2.4, 4.0], components=components)
    if everything:   # GWB + white noise + ECORR on top; else red noise alone
        eng.set_white_noise(efac=[1.1, 0.9, 1.3], log10_equad=[-6.5, -6.8, -6.2])
        eng.set_jitter(log10_ecorr=[-6.6, -6.9, -6.4], coarsegrain=0.1)
        eng.set_gwb(-14.4, 13. / 3.)
    eng.prepare()
    assert eng.K == 2 * components
    for R in (1, 16, 19):
        eng.synth_variant = 2
        ref = eng.generate(R, r0=7).clone()
        eng.synth_variant = 0
        got = eng.generate(R, r0=7)
        assert ref.shape == (R, sum(COUNTS)) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        assert torch.equal(got, ref), (components, everything, R)
