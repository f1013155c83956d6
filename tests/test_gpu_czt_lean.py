"""The chirp-z kernel's twiddle / pruning ladder steps (FUSE bits 16, 32, 64 of k_gwb_czt) remove work, not roundings: every one of
them, alone on top of the fused kernel (variant 10 + 15), all together, and the default's choice of them (variant 0), must give the
bits of variant 25."""
import numpy as np
import pytest

from oracle import pta_oracle as po

pytestmark = pytest.mark.gpu

BASE = 10 + 15                                            # the fused kernel without the new bits
LEAN = [0, 10 + 15 + 16, 10 + 15 + 32, 10 + 15 + 64, 10 + 127]   # the default, each bit alone, all three
# (2000, 1100): the window [9, 1109) crosses 1024, the last butterfly keeps its full form; (500, 37): only output 0 is ever stored
# (3499, 600): the last shape that fits, Kf + npts - 2 = 4095; (1026, 1015), (700, 1016), (700, 1017): the window ends at 1023, 1024,
# 1025 - the pruned last butterfly's last shape and the full one's first two; (513 .. 515, 40): Kf = 511, 512, 513 around the one
# 512-block of the first butterfly that straddles Kf.  tests/test_gpu_gwb_direct.py repeats the comparison at i0 other than 10.
SHAPES = [(3000, 600), (3001, 600), (601, 200), (500, 37), (2400, 601), (3400, 600), (2000, 1100),
          (3499, 600), (1026, 1015), (700, 1016), (700, 1017), (513, 40), (514, 40), (515, 40)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(torch=torch, lib=_lib, dv=dv, s=dv.stream_ptr())


def _setup(gpu, Nf, npts, dt):
    dv, lib = gpu["dv"], gpu["lib"]
    rng = np.random.default_rng(Nf)
    C = rng.uniform(0.5, 2.0, Nf) * 1e-14
    sq_d = dv.f64(C ** 0.5)
    tabs = [dv.empty((8192,)), dv.empty((8192,)), dv.empty((8192,)), dv.empty((2 * npts,))]
    lib.call("pta_gwb_czt_setup", dv.ptr(sq_d), Nf, npts, 10, 1.0 / dt, *[dv.ptr(x) for x in tabs], gpu["s"])
    return rng, C, sq_d, tabs


@pytest.mark.parametrize("Nf,npts", SHAPES)
def test_lean_variants_bit_identical_to_fused_kernel(gpu, Nf, npts):
    """replay form and on-chip-draw form (recipe of test_gwb_chirp_z_fft_vs_numpy_and_vs_dft_gemm, R = 2, P = 3): variants 0, 10+15+16,
    10+15+32, 10+15+64, 10+127 == variant 25 bit for bit; variant 0 within 1e-12 of NumPy's Hermitian-packed ifft."""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    assert lib.lib.pta_gwb_czt_fits(Nf, npts, 10) == 1
    seed, r0, R, P = 99, 12345, 2, 3
    M = R * P
    dt = 977.0
    rng, C, sq_d, tabs = _setup(gpu, Nf, npts, dt)
    w = rng.standard_normal((M, Nf, 2))
    w_d = dv.f64(w)
    tp = [dv.ptr(x) for x in tabs]

    def run(variant, replay):
        G = dv.zeros((M, npts))
        if replay:
            lib.call("pta_gwb_czt", 0, 0, dv.ptr(w_d), 2 * Nf, R, P, Nf, npts, 10, *tp, dv.ptr(G), npts, variant, 0, gpu["s"])
        else:
            lib.call("pta_gwb_czt", seed, r0, None, 0, R, P, Nf, npts, 10, *tp, dv.ptr(G), npts, variant, 0, gpu["s"])
        return G

    for replay in (True, False):
        base = run(BASE, replay)
        assert float(base.abs().max()) > 0
        for variant in LEAN:
            assert torch.equal(run(variant, replay), base), (variant, replay)
    Res_f = (w[..., 0] + 1j * w[..., 1]) * C ** 0.5
    Res_f[:, 0] = 0; Res_f[:, -1] = 0
    ref = po.gwb_time_series(Res_f, dt)[:, 10:npts + 10]
    assert np.max(np.abs(run(0, True).cpu().numpy() - ref)) < 1e-12 * np.max(np.abs(ref))


def test_scaled_default_against_cross_check(gpu):
    """pta_gwb_czt_scaled: variant 0 (the lean fused kernel) against variant 1 (every stage through LDS, table twiddles) at the
    1e-12 of the chirp-z tests; with a scale of exactly 1 the scaled kernel gives the bits of the unscaled one."""
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    Nf, npts, seed, r0, R, P = 3001, 600, 99, 12345, 2, 3
    M = R * P
    rng, C, sq_d, tabs = _setup(gpu, Nf, npts, 977.0)
    tp = [dv.ptr(x) for x in tabs]
    ld = Nf + 3
    scale = dv.f64(rng.uniform(0.2, 3.0, (R, ld)))
    out = []
    for variant in (0, 1):
        G = dv.zeros((M, npts))
        lib.call("pta_gwb_czt_scaled", seed, r0, None, 0, R, P, Nf, npts, 10, *tp, dv.ptr(G), npts, variant, 0, dv.ptr(scale), ld, gpu["s"])
        out.append(G.cpu().numpy())
    assert np.max(np.abs(out[0])) > 0
    assert np.max(np.abs(out[0] - out[1])) < 1e-12 * np.max(np.abs(out[1]))
    ones = dv.f64(np.ones((R, ld)))
    G1, G = dv.zeros((M, npts)), dv.zeros((M, npts))
    lib.call("pta_gwb_czt_scaled", seed, r0, None, 0, R, P, Nf, npts, 10, *tp, dv.ptr(G1), npts, 0, 0, dv.ptr(ones), ld, gpu["s"])
    lib.call("pta_gwb_czt", seed, r0, None, 0, R, P, Nf, npts, 10, *tp, dv.ptr(G), npts, BASE, 0, gpu["s"])
    assert torch.equal(G1, G)
