"""The rows buffer the optimal statistic, the likelihood and the F-statistic share (engine_stats.StatisticsMixin): the three
generate_* calls in turn on one engine, with chunks that leave a short last chunk and make the buffer grow, against the statistics
of generate()'s rows - bit for bit - and the first call repeated after the others have used the buffer."""
import numpy as np
import pytest
import torch

from test_os_matched_host import _engine as _configured

pytestmark = pytest.mark.gpu


def test_one_rows_buffer_serves_the_three_statistics():
    eng = _configured()                                   # four pulsars of c3_mini: white noise, red noise with pulsar 1 None
    eng.set_jitter(log10_ecorr=-6.5, coarsegrain=0.1)
    eng.set_gwb(-14.4, 13. / 3.)
    eng.prepare_optimal_statistic(components=6, matched=True)
    eng.prepare_likelihood(components=6)
    eng.prepare_f_statistic([5.1e-9, 1.21e-8, 2.33e-8], sky=(np.array([-0.2, 0.44]), np.array([1.9, 4.4])))
    grid, _ = eng.theta_grid(gwb_log10_A=[-14.6, -14.2])

    os1 = eng.generate_os(5, chunk=2)                     # three chunks, the last one short
    assert eng._stats_rows.shape[0] == 2
    lnl = eng.generate_lnl(3, grid, chunk=3)
    fs = eng.generate_f_statistic(7, chunk=4)             # the buffer has to grow
    os2 = eng.generate_os(5, chunk=2)
    assert torch.equal(os2["A2"], os1["A2"]) and torch.equal(os2["snr"], os1["snr"])

    ref = eng.optimal_statistic(eng.generate(5))
    assert torch.equal(os1["A2"], ref["A2"]) and torch.equal(os1["snr"], ref["snr"])
    assert torch.equal(lnl["lnl"], eng.log_likelihood(eng.generate(3), grid)["lnl"])
    ref = eng.f_statistic(eng.generate(7))
    assert torch.equal(fs["fp"], ref["fp"]) and torch.equal(fs["fe"], ref["fe"])
    assert bool(torch.isfinite(os1["A2"]).all()) and bool(torch.isfinite(lnl["lnl"]).all()) and bool(torch.isfinite(fs["fe"]).all())

    assert not any(hasattr(eng, name) for name in ("_os_rows", "_lnl_rows", "_fs_rows"))
    assert eng._stats_rows.shape == (eng._stats_rows.shape[0], eng.n_toa) and eng._stats_rows.shape[0] >= 4
    buffers = [k for k, v in vars(eng).items() if k.endswith("_rows") and isinstance(v, torch.Tensor)]
    assert buffers == ["_stats_rows"], buffers
