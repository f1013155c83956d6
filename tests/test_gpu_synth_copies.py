"""The four copies of the fused synthesis kernel's MFMA variant (synth_variant 16 + 16 noidx + 32 generic: scalar row offsets or per-lane
index products in the red-noise loop, the straight-line epilogue compiled for a plan with GWB, white noise and ECORR or the epilogue for
any plan) and the default (synth_variant 0, which picks among them) against one of them, the kernel as it was before the copies
(synth_variant 48): the same loads, the same arithmetic - the same bits, at the small shapes at which the copies can differ (a single
clamped lane, a tile less or plus one TOA, a partial realisation group, a counter offset beyond 2^32).  Values of synth_variant
without a kernel, those of the retired prefetch and 3-per-CU instances among them, are refused.

The host guard that sends a plan beyond the 32-bit lane offsets to the per-lane index products needs rn_k ldf 8 >= 2^32 (a design
matrix of 4 GB): tests/test_gpu_synth_direct.py::test_lane_offset_guard runs both sides of it, with a direct call, two or four bins and
a leading dimension of 2^28 or 2^27, against the host reference.  The noidx bit of the variant runs the same loads."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = 48                              # scalar row offsets, the copy for any plan: the kernel as it was
VARIANTS = [16, 32]                    # 16 + 16 noidx: the copy for a complete plan where the plan is complete, either addressing
# + 32: the copy compiled for any plan (requests inside `if (has_gw)` ...) also where the plan is complete and its own copy would run
VARIANTS_GENERIC = [64]
VARIANTS_SINGLE = [16, 32]             # wn_mode "single" has the same four copies (at 3 workgroups per CU)
COUNTS = (1, 255, 256, 257, 300)       # a single clamped lane, a tile less one, a full tile, a tile plus one TOA, a short last tile
BATCHES = ((1, 0), (16, 0), (17, 0), (17, 2 ** 32 - 3))   # (R, r0): 17 = a partial realisation group


def make_psrs(counts, seed, unsorted=()):
    from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal
    rng = np.random.default_rng(seed)
    out = []
    for a, n in enumerate(counts):
        mjd = rng.uniform(53000, 57500, n)
        if a not in unsorted:
            mjd = np.sort(mjd)
        p = SimulatedPulsar(toas=ArrayTOAs(mjd, 0.5), name=f"J{a:04d}",
                            loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
        make_ideal(p)
        out.append(p)
    return out


@pytest.fixture(scope="module")
def psrs():
    return make_psrs(COUNTS, 31)


def engine(psrs, rn=30, rn_skip=None, wn=True, ec=True, gw=True):
    from pta_replicator_amd.engine import ReplicaEngine
    P = len(psrs)
    eng = ReplicaEngine(psrs, seed=9876)
    eng.td_warmup = False
    if rn:
        # (a pulsar of one TOA has no time span, hence no red-noise spectrum: it goes without - as a lane clamped to a single TOA it still
        # runs the rotation, with zero coefficients)
        A = [-13.8 - 0.1 * a if len(p.toas.get_mjds()) > 1 else None for a, p in enumerate(psrs)]
        if rn_skip is not None:
            A[rn_skip] = None
        eng.set_red_noise(A, [3.1 + 0.2 * a for a in range(P)], components=rn)
    if wn:
        eng.set_white_noise(efac=[1.1 - 0.05 * a for a in range(P)], log10_equad=[-6.5 - 0.1 * a for a in range(P)])
    if ec:
        eng.set_jitter(log10_ecorr=[-6.6 - 0.1 * a for a in range(P)], coarsegrain=0.1)
    if gw:
        eng.set_gwb(-14.4, 13. / 3.)
    eng.prepare()
    return eng


def check(eng, variants, batches=BATCHES, default_too=False):
    import torch
    n = eng.n_toa
    for R, r0 in batches:
        eng.synth_variant = BASE
        ref = eng.generate(R, r0=r0).clone()
        assert ref.shape == (R, n) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        for v in list(variants) + ([0] if default_too else []):
            eng.synth_variant = v
            got = eng.generate(R, r0=r0)
            assert torch.equal(got, ref), (v, R, r0)
    eng.synth_variant = 0


def test_everything_and_default(psrs):
    """GWB + red noise (K = 60: K % 4 == 0) + EFAC/EQUAD + staged ECORR; the default variant too; rows with ld_out > n_toa."""
    import torch
    from pta_replicator_amd import device as dv
    eng = engine(psrs)
    assert eng.K == 60
    check(eng, VARIANTS + VARIANTS_GENERIC, default_too=True)
    # padded output rows: nothing is written beyond n_toa
    R, pad = 17, 5
    eng.synth_variant = BASE
    ref = eng.generate(R, r0=3).clone()
    for v in VARIANTS + [0]:
        buf = dv.empty((R, eng.n_toa + pad))
        buf.fill_(-7.25)
        eng.synth_variant = v
        eng.generate(R, r0=3, out=buf[:, :eng.n_toa])
        assert torch.equal(buf[:, :eng.n_toa], ref), v
        assert bool((buf[:, eng.n_toa:] == -7.25).all()), v
    eng.synth_variant = 0


def test_tail_clamp_loop_and_a_pulsar_without_red_noise(psrs):
    """29 components: K = 58, the K % 4 != 0 loop of the rotation; pulsar 2 (a full tile) has no red noise."""
    eng = engine(psrs, rn=29, rn_skip=2)
    assert eng.K == 58
    check(eng, VARIANTS)


@pytest.mark.parametrize("off", ["rn", "gw", "wn", "ec"])
def test_one_group_of_operands_absent(psrs, off):
    """an engine without red noise (no rotation), without GWB, without white noise, without ECORR: each drops a group of operands,
    and the kernels compiled for a complete plan are not the ones launched."""
    eng = engine(psrs, rn=0 if off == "rn" else 30, wn=off != "wn", ec=off != "ec", gw=off != "gw")
    check(eng, VARIANTS, batches=BATCHES[1:])


def test_ecorr_epochs_beyond_the_staging_buffer():
    """300 TOAs in random order: a tile's epochs span more pairs than the staging buffer holds, the deviates are drawn per TOA"""
    from pta_replicator_amd import _lib
    eng = engine(make_psrs((300, 17), 5, unsorted=(0,)))
    epn = eng.d_tiles[4].cpu().numpy()
    assert epn[0] == 0 and epn[-1] > 0, epn       # pulsar 0's tiles are not staged (> ENGINE_EPMAX pairs), pulsar 1's is
    assert _lib.ENGINE_EPMAX < 150
    check(eng, VARIANTS, batches=BATCHES[2:])


def test_single_deviate_white_noise(psrs):
    eng = engine(psrs)
    eng.wn_mode = "single"
    check(eng, VARIANTS_SINGLE + [v + 32 for v in VARIANTS_SINGLE], batches=BATCHES[1:])
    eng.synth_variant = 16 + 5 + 8   # a retired prefetch instance: refused, not replaced
    with pytest.raises(Exception):
        eng.generate(2)
    eng.synth_variant = 0


def test_rng_fast(psrs):
    eng = engine(psrs)
    eng.rng_fast = 1
    check(eng, VARIANTS, batches=BATCHES[1:])


def test_variants_without_a_kernel_are_refused(psrs):
    import torch
    eng = engine(psrs, gw=False)
    # 20, 21, 17, 27: never had a kernel; 18, 24, 50: one per retired bit (rotation prologue, 3 workgroups per CU, the prologue on the
    # generic copy); 4, 8: the all-VALU kernel at other register budgets
    for v in (16 + 4, 16 + 5, 16 + 1, 16 + 3 + 8, 18, 24, 50, 4, 8):
        eng.synth_variant = v
        with pytest.raises(Exception):
            eng.generate(2)
        eng.synth_variant = 0
        out = eng.generate(2)
        assert out.shape == (2, eng.n_toa) and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0, v
