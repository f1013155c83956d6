"""The interpolation tail of the GWB chain called directly: pta_gwb_bracket, pta_gwb_weights and pta_gwb_interp against the header's
contract evaluated in long double - numpy.interp's bracket and its two-term expression slope (x - xp[j]) + fp[j], which is what
numpy.interp computes between two nodes (numpy itself has no long double form of it).

TOAs before the first node, on it, exactly on interior nodes, on the last node and after it, unsorted, N no multiple of the 256
threads of a workgroup; grids of 2 and more samples, uniform and not; R > 1 with ld_out > N and ldg > npts, NaN in every padding
element before and after; accumulate 0 and 1, scale 1 and 1 / 86400.

  bracket  exact: the last j with ut[j] <= t, clamped to [0, npts - 2]
  weights  (t - ut[j]) / (ut[j+1] - ut[j]): two differences and a quotient, one rounding each:            3.1 u |w|
  interp   slope = dG / dut (3 roundings), x - ut[j] (1), their product (1), the sum (1), the scale (1), the accumulation (1):
           u (5.1 |slope dx| + |v|) |scale| [+ u |v scale| with a scale] [+ u |out| when accumulating], a worst case that a single
           rounding of a sum can reach where slope dx is small (the 1.01 on the last three terms is their second order; measured
           up to 0.99) - and where a TOA sits on
           node j <= npts - 2, dx is exactly 0 and the value is G[j] (times the scale, rounded once) exactly.  On the LAST node the
           bracket is npts - 2 by the contract's clamp, so the value is the two-term expression at dx = one full step: within the
           bound of G[npts - 1], not bit-equal to it.  Outside the grid the contract's expression extrapolates on the first or last
           interval."""
import numpy as np
import pytest

from synth_reference import HAVE_LONG_DOUBLE, L, U

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not HAVE_LONG_DOUBLE, reason="no 80-bit long double on this host")]

# (npts, N, R, P, uniform grid)
SHAPES = [(2, 5, 1, 1, True), (2, 300, 3, 2, True), (3, 257, 2, 3, False), (600, 1000, 3, 4, True), (601, 255, 1, 5, False),
          (37, 513, 2, 1, True)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pta_replicator_amd import _lib, device as dv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(torch=torch, lib=_lib, dv=dv, s=dv.stream_ptr())


def _case(npts, N, P, uniform):
    rng = np.random.default_rng([npts, N, P])
    ut = 4.6e9 + 977.0 * 3600.0 * np.arange(npts)
    if not uniform:
        ut[1:] += rng.uniform(-0.3, 0.3, npts - 1) * 977.0 * 3600.0
    step = ut[1] - ut[0]
    t = rng.uniform(ut[0], ut[-1], N)
    special = [ut[0] - 0.37 * step, ut[0], ut[-1], ut[-1] + 0.41 * step, np.nextafter(ut[0], -np.inf), np.nextafter(ut[-1], np.inf),
               np.nextafter(ut[-1], -np.inf)]
    special += list(ut[1:-1][:: max(1, (npts - 2) // 7)]) + [np.nextafter(x, -np.inf) for x in ut[1:-1][:3]]
    special = np.array(special[:N])
    t[rng.permutation(N)[:len(special)]] = special      # scattered, so the TOAs are unsorted with or without them
    psr = rng.integers(0, P, N)
    return ut, t, psr, rng


def _bracket(ut, t):
    return np.clip(np.searchsorted(ut, t, side="right") - 1, 0, len(ut) - 2)


@pytest.mark.parametrize("npts,N,R,P,uniform", SHAPES)
def test_bracket_and_weights(gpu, npts, N, R, P, uniform):
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    ut, t, _, _ = _case(npts, N, P, uniform)
    ut_d, t_d = dv.f64(ut), dv.f64(t)
    jlo = torch.full((N + 3,), -7, dtype=torch.int32, device="cuda")
    lib.call("pta_gwb_bracket", dv.ptr(ut_d), npts, dv.ptr(t_d), N, dv.ptr(jlo), gpu["s"])
    j = jlo.cpu().numpy()
    want = _bracket(ut, t)
    assert np.array_equal(j[:N], want) and np.all(j[N:] == -7)
    w = torch.full((N + 3,), float("nan"), dtype=torch.float64, device="cuda")
    lib.call("pta_gwb_weights", dv.ptr(ut_d), npts, dv.ptr(t_d), dv.ptr(jlo), N, dv.ptr(w), gpu["s"])
    got = w.cpu().numpy()
    ref = (t.astype(L) - ut[want].astype(L)) / (ut[want + 1].astype(L) - ut[want].astype(L))
    assert np.all(np.isnan(got[N:])) and np.all(np.isfinite(got[:N]))
    frac = float(np.max(np.abs(got[:N].astype(L) - ref).astype(np.float64) / (3.1 * U * np.abs(ref).astype(np.float64) + 1e-300)))
    print(f"weights npts={npts} N={N}: {frac:.3f} of the bound")
    assert frac <= 1.0
    on = t == ut[want]
    assert on.sum() >= 1 and np.all(got[:N][on] == 0.0) and np.all(got[:N][t == ut[-1]] == 1.0)
    assert np.all(got[:N][t < ut[0]] < 0.0) and np.all(got[:N][t > ut[-1]] > 1.0)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 1.0 / 86400.0])
@pytest.mark.parametrize("npts,N,R,P,uniform", SHAPES)
def test_interp(gpu, npts, N, R, P, uniform, scale, accumulate):
    dv, lib, torch = gpu["dv"], gpu["lib"], gpu["torch"]
    ut, t, psr, rng = _case(npts, N, P, uniform)
    j = _bracket(ut, t)
    ldg, ld_out = npts + 3, N + 5
    G = np.full((R * P + 1, ldg), np.nan)
    G[:R * P, :npts] = rng.standard_normal((R * P, npts))
    out0 = np.full((R + 1, ld_out), np.nan)
    out0[:R, :N] = rng.standard_normal((R, N))
    out = dv.f64(out0)
    hold = [dv.f64(G), dv.f64(ut), dv.f64(t), dv.i32(psr), dv.i32(j)]
    lib.call("pta_gwb_interp", dv.ptr(hold[0]), ldg, P, npts, dv.ptr(hold[1]), dv.ptr(hold[2]), dv.ptr(hold[3]), dv.ptr(hold[4]), N, R,
             scale, dv.ptr(out), ld_out, accumulate, gpu["s"])
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[R])) and np.all(np.isnan(got[:R, N:])) and np.all(np.isfinite(got[:R, :N]))
    rows = (np.arange(R)[:, None] * P + psr[None, :])
    g0, g1 = G[rows, j[None, :]].astype(L), G[rows, j[None, :] + 1].astype(L)
    dx = (t.astype(L) - ut[j].astype(L))[None, :]
    t1 = (g1 - g0) / (ut[j + 1].astype(L) - ut[j].astype(L))[None, :] * dx
    v = (t1 + g0) * L(scale)
    ref = v + out0[:R, :N].astype(L) if accumulate else v
    b = U * ((5.1 * np.abs(t1) + 1.01 * np.abs(t1 + g0)) * abs(scale) + (1.01 * np.abs(v) if scale != 1.0 else 0)
             + (1.01 * np.abs(ref) if accumulate else 0))
    err = np.abs(got[:R, :N].astype(L) - ref)
    frac = float(np.max((err / np.maximum(b, L(1e-300))).astype(np.float64)))
    print(f"interp npts={npts} N={N} R={R} scale={scale:.3g} accumulate={accumulate}: {frac:.3f} of the bound")
    assert frac <= 1.0
    on = t == ut[j]                                     # on node j <= npts - 2: the node's value, exactly
    node = G[rows, j[None, :]][:, on]
    exact = node * scale if scale != 1.0 else node
    exact = out0[:R, :N][:, on] + exact if accumulate else exact
    assert on.sum() >= 1
    if not (accumulate and scale != 1.0):               # (there v scale + out may be one fused operation or two: the bound alone)
        assert np.array_equal(got[:R, :N][:, on], exact)
