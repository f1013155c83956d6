"""pta_gwb_mix variant 0 (k_gwb_mix_stream: resident grid, requests one item ahead, the factor's zero triangle skipped) against
variant 3 (k_gwb_mix_small, what variant 0 was) bit for bit, and both against NumPy within test_gwb_mix_against_numpy's bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(torch=torch, lib=_lib, dv=dv, s=dv.stream_ptr())


def _mix(gpu, M_d, P, G0_d, R, npts, ldg, variant):
    dv, lib = gpu["dv"], gpu["lib"]
    G_d = gpu["torch"].full((R, P, ldg), SENTINEL, dtype=gpu["torch"].float64, device="cuda")
    lib.call("pta_gwb_mix", dv.ptr(M_d), P, dv.ptr(G0_d), R, npts, ldg, dv.ptr(G_d), variant, gpu["s"])
    return G_d


def _check(gpu, P, npts, R, rng):
    dv, torch = gpu["dv"], gpu["torch"]
    ldg = npts + 3
    M = np.tril(rng.standard_normal((P, P)))
    G0 = rng.standard_normal((R, P, ldg))
    M_d, G0_d = dv.f64(M), dv.f64(G0)
    new, old = _mix(gpu, M_d, P, G0_d, R, npts, ldg, 0), _mix(gpu, M_d, P, G0_d, R, npts, ldg, 3)
    assert torch.equal(new, old), (P, npts, R)                       # padding columns included
    ref = np.einsum("ab,rbj->raj", M, G0[:, :, :npts])
    bound = 1e-13 * max(1.0, np.max(np.abs(ref)))
    for G_d in (new, old):
        G = G_d.cpu().numpy()
        assert np.max(np.abs(G[:, :, :npts] - ref)) < bound, (P, npts, R)
        assert np.all(G[:, :, npts:] == SENTINEL), (P, npts, R)      # the sentinel in the padding survives
    return M, G0_d, new


@pytest.mark.parametrize("P", [1, 3, 16, 17, 40, 49, 68, 80])      # 40, 49: three and four pulsar tiles, which no other size reaches
def test_stream_equals_small_and_numpy(gpu, P):
    """Every npts in {1, 63, 64, 65, 600} x R in {1, 4, 5, 9} with ldg = npts + 3: fewer items than waves, ragged last chunk, one
    to five pulsar tiles, whole and partial last K-steps."""
    rng = np.random.default_rng(4100 + P)
    for npts in (1, 63, 64, 65, 600):
        for R in (1, 4, 5, 9):
            _check(gpu, P, npts, R, rng)


@pytest.mark.parametrize("P,npts,R,wg_per_cu", [(68, 600, 330, 3), (17, 65, 5000, 8)])
def test_stream_walks_several_items_per_wave(gpu, P, npts, R, wg_per_cu):
    """More items (R x ceil(npts / 16)) than the resident grid has waves: three and more per wave, so both register sets, the step
    (dr, dc) with its carry, and both copies of the last item run.  wg_per_cu bounds the grid from above: 3 workgroups of 43.5 KB
    fit a CU's 160 KB of LDS at P = 68, 8 are the most a CU holds of any 256-thread kernel."""
    info = gpu["dv"].device_info()
    assert R * ((npts + 15) // 16) > 2 * wg_per_cu * 4 * info["cu_count"], info     # more than two full rounds
    _check(gpu, P, npts, R, np.random.default_rng(4200 + P))


@pytest.mark.parametrize("P", [68, 17, 3])
def test_upper_triangle_of_the_input_is_not_read(gpu, P):
    """NaN above the diagonal of the *input* factor changes nothing: the triangle is staged as zeros and its K-steps are skipped.
    (Variant 3 multiplies by whatever the input holds there, so it is not run on this factor.)"""
    dv, torch = gpu["dv"], gpu["torch"]
    npts, R = 65, 5
    M, G0_d, clean = _check(gpu, P, npts, R, np.random.default_rng(4300 + P))
    Mn = M.copy()
    Mn[np.triu_indices(P, 1)] = np.nan
    dirty = _mix(gpu, dv.f64(Mn), P, G0_d, R, npts, npts + 3, 0)
    assert torch.equal(dirty, clean)
