"""pta_gwb_czt_fits on the host (no launch, no GPU): the chirp-z form fits when the lags j - k, Kf + npts - 1 of them, fit one 4096-point
convolution AND the window's own outputs i0 - 1 .. i0 + npts - 2 lie inside it.  Before the second condition a window beyond 4095
was accepted: k_czt_setup's positive lags then claimed the slots of the negative ones and the kernel's last butterfly indexed past
its plane, or stored nothing at all."""
import gwb_cases as gc


def test_czt_fits_is_the_contract():
    from pta_replicator_amd import _lib
    fits = _lib.lib.pta_gwb_czt_fits
    assert (fits(600, 600, 3600), fits(3499, 600, 10), fits(3500, 600, 10)) == (0, 1, 0)
    for Nf in (2, 3, 4, 600, 3498, 3499, 3500, 4098, 4099, 2 ** 31 - 1):
        for npts in (-1, 0, 1, 2, 599, 600, 601, 4095, 4096, 4097, 2 ** 31 - 1):
            for i0 in (-1, 0, 1, 2, 10, 3496, 3497, 3498, 4095, 4096, 4097, 2 ** 31 - 1):
                assert fits(Nf, npts, i0) == int(gc.czt_fits(dict(Nf=Nf, npts=npts, i0=i0))), (Nf, npts, i0)
    for c in gc.CASES:
        assert fits(c["Nf"], c["npts"], c["i0"]) == int(gc.czt_fits(c)) == int(c["name"] != "C-i0-0"), c["name"]
