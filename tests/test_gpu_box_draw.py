"""The five uniform entries (pta_hyper_uniform, pta_hyper_uniform_field, pta_cw_uniform, pta_cw_catalog_uniform, pta_bwm_uniform) rest on
one kernel (pta_box_kernels.hip): the identities between them that the headers promise, and every entry bit for bit against the Philox
reference mapped through lo + (hi - lo) u2 with ONE rounding (exact rational arithmetic rounded once: math.fma's value)."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import philox_ref

pytestmark = pytest.mark.gpu

R, R0, SEED, S = 3, 2 ** 32 + 3, 0x9E3779B97F4A7C15, 3
HYPER, CW, BWM = 7, 8, 9          # stream kinds (pta_rng.h)
N_CW, N_BWM = 8, 5                # label columns of a CW source and of a burst


def _fma(a, b, c):
    """a * b + c rounded once, elementwise"""
    return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, np.broadcast_to(c, a.shape))])


def _want(kind, field, lo, hi):
    """[R, n] reference table of stream (kind, field)"""
    sid = philox_ref.stream_id(kind, field)
    return np.stack([_fma(hi - lo, philox_ref.uniform_pairs(SEED, R0 + r, sid, len(lo))[1], lo) for r in range(R)])


@pytest.mark.parametrize("n_par", [1, 257])
def test_uniform_entries_bit_for_bit(n_par):
    from pta_replicator_amd import _lib, device as dv
    rng = np.random.default_rng(n_par)
    n = max(n_par, N_CW)           # the catalogue and the burst read the first 8 and 5 boxes
    lo = rng.uniform(-20.0, 5.0, n)
    hi = lo + rng.uniform(1e-3, 30.0, n)
    d_lo, d_hi, s = dv.f64(lo), dv.f64(hi), dv.stream_ptr()

    def table(entry, shape, *mid):
        out = dv.empty(shape)
        _lib.call(entry, SEED, R0, R, *mid, dv.ptr(d_lo), dv.ptr(d_hi), dv.ptr(out), s)
        return out.cpu().numpy()
    hyper = table("pta_hyper_uniform", (R, n_par), n_par)
    field0 = table("pta_hyper_uniform_field", (R, n_par), n_par, 0)
    field4 = table("pta_hyper_uniform_field", (R, n_par), n_par, 4)
    cw = table("pta_cw_uniform", (R, n_par), n_par)
    cat = table("pta_cw_catalog_uniform", (R, S, N_CW), S)
    bwm = table("pta_bwm_uniform", (R, N_BWM))
    # the identities between the entries
    assert np.array_equal(field0, hyper)
    k = min(n_par, N_CW)
    assert np.array_equal(cat[:, 0, :k], cw[:, :k])
    # every entry against the reference draw
    assert np.array_equal(hyper, _want(HYPER, 0, lo[:n_par], hi[:n_par]))
    assert np.array_equal(field4, _want(HYPER, 4, lo[:n_par], hi[:n_par]))
    assert np.array_equal(cw, _want(CW, 0, lo[:n_par], hi[:n_par]))
    for src in range(S):
        assert np.array_equal(cat[:, src], _want(CW, src, lo[:N_CW], hi[:N_CW])), src
    assert np.array_equal(bwm, _want(BWM, 0, lo[:N_BWM], hi[:N_BWM]))
