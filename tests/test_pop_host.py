"""CPU checks of the population path: the Poisson sampler of csrc/pta_pop.h compiled with g++ (tests/pop/pop_host.cpp) against its NumPy
twin (tests/pop_reference.py) and against the Poisson distribution, the selection twin against the reference's record, the host tables
of _pop.make_tables against np.digitize, and every refusal of set_population / population_theta on an engine that is configured but not
prepared (no GPU needed: every refusal happens before anything is launched)."""
import numpy as np
import pytest
from scipy import stats

import pop_reference as pr
from pop_cases import (FLAG_CAP, LAMBDAS, NORMAL_LAMBDAS, SEED, RecordHelpers, build_host, draws, engine, host_poisson, host_z0, record,
                       synthetic, user_spec)

N_DRAWS = 200_000


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("pop"))


@pytest.fixture(scope="module")
def sampled(ph):
    """{lambda: (N of the g++ build, attempts)} for 2e5 (realisation, cell) draws each, computed once"""
    rho, cell = draws(N_DRAWS, r0=(1 << 32) + 3)
    return {lam: host_poisson(ph, SEED, rho, cell, np.full(N_DRAWS, lam)) for lam in LAMBDAS + NORMAL_LAMBDAS[:2]}, rho, cell


def _compare(n_host, n_twin, flag, what):
    frac = flag.mean()
    bad = np.flatnonzero((n_host != n_twin) & ~flag)
    print(f"{what}: flagged {flag.sum()} of {len(flag)} ({frac:.2e}), mismatches among the flagged {np.count_nonzero((n_host != n_twin) & flag)}, "
          f"among the rest {len(bad)}")
    assert frac <= FLAG_CAP, (what, frac)
    assert len(bad) == 0, (what, bad[:5], n_host[bad[:5]], n_twin[bad[:5]])


@pytest.mark.parametrize("lam", LAMBDAS)
def test_header_matches_the_twin_at_fixed_rates(ph, sampled, lam):
    draws_of, rho, cell = sampled
    n_twin, flag, att_twin = pr.poisson(SEED, rho, cell, np.full(N_DRAWS, lam))
    _compare(draws_of[lam][0], n_twin, flag, f"lambda = {lam}")
    same = ~flag
    assert np.array_equal(draws_of[lam][1][same], att_twin[same])
    assert ph.ph_regime(lam) == (0 if lam == 0 else 1 if lam < 10 else 2)


def test_header_matches_the_twin_at_log_uniform_rates(ph):
    rho, cell = draws(N_DRAWS, r0=7, per_real=1000)
    lam = 10 ** np.random.default_rng(5).uniform(-6.0, np.log10(float(1 << 20)), N_DRAWS)
    lam = np.minimum(lam, np.nextafter(float(1 << 20), 0.0))
    n_twin, flag, _ = pr.poisson(SEED, rho, cell, lam)
    _compare(host_poisson(ph, SEED, rho, cell, lam)[0], n_twin, flag, "log-uniform lambda over [1e-6, 2^20)")


@pytest.mark.parametrize("lam", NORMAL_LAMBDAS)
def test_normal_regime_is_exact(ph, lam):
    """lambda >= 2^20: no exp, log or lgamma, only the project's Box-Muller deviate (the g++ build's own, handed to the twin) through
    IEEE sqrt, *, + and floor: every draw equal, no borderline rule"""
    rho, cell = draws(N_DRAWS, r0=(1 << 40) + 1)
    lams = np.full(N_DRAWS, lam)
    n_twin, flag, _ = pr.poisson(SEED, rho, cell, lams, z0=host_z0(ph, SEED, rho, cell))
    n_host, att = host_poisson(ph, SEED, rho, cell, lams)
    assert not flag.any() and np.array_equal(n_host, n_twin) and np.all(att == 1) and ph.ph_regime(lam) == 3
    # and the deviate is the stream's: philox_ref's libm Box-Muller of the same block agrees to rounding
    n_libm, _, _ = pr.poisson(SEED, rho, cell, lams)
    assert np.max(np.abs(n_libm - n_host)) <= 1 + 4 * np.spacing(lam)


@pytest.mark.parametrize("lam", [x for x in LAMBDAS if x > 0] + list(NORMAL_LAMBDAS[:2]))
def test_draws_follow_the_poisson_distribution(sampled, lam):
    n = sampled[0][lam][0]
    m = len(n)
    mean, var = n.mean(), n.var(ddof=1)
    se_mean, se_var = np.sqrt(lam / m), np.sqrt((lam + 2 * lam ** 2) / m)   # a Poisson's fourth central moment is lam + 3 lam^2
    print(f"lambda = {lam}: mean - lambda = {(mean - lam) / se_mean:+.2f} se, variance - lambda = {(var - lam) / se_var:+.2f} se")
    assert abs(mean - lam) <= 5 * se_mean
    assert abs(var - lam) <= 5 * se_var
    if lam <= 37.5:
        hi = int(n.max()) + 1
        expect = m * stats.poisson.pmf(np.arange(hi + 1), lam)
        expect[hi] = m * stats.poisson.sf(hi - 1, lam)            # the last cell takes the tail
        obs = np.bincount(n.astype(np.int64), minlength=hi + 1).astype(np.float64)
        pooled_o, pooled_e, o, e = [], [], 0.0, 0.0
        for oi, ei in zip(obs, expect):                           # pool neighbours until a cell expects >= 10
            o, e = o + oi, e + ei
            if e >= 10:
                pooled_o.append(o), pooled_e.append(e)
                o = e = 0.0
        if pooled_e:
            pooled_o[-1] += o
            pooled_e[-1] += e
        else:
            pooled_o, pooled_e = [o], [e]
        pooled_o, pooled_e = np.array(pooled_o), np.array(pooled_e)
        if len(pooled_e) > 1:
            chi2 = float(np.sum((pooled_o - pooled_e) ** 2 / pooled_e))
            bound = stats.chi2.ppf(1 - 1e-6, len(pooled_e) - 1)
            print(f"lambda = {lam}: chi2 = {chi2:.1f} over {len(pooled_e)} cells, bound {bound:.1f}")
            assert chi2 < bound


def test_ptrs_attempts_at_the_lower_edge(sampled):
    att = sampled[0][10.0][1]
    print("mean PTRS attempts at lambda = 10:", att.mean(), "max", att.max())
    assert att.mean() < 1.5 and att.max() < 64


def test_zero_rate_draws_nothing(ph):
    rho, cell = draws(1000)
    n, att = host_poisson(ph, SEED, rho, cell, np.zeros(1000))
    assert not n.any() and not att.any()


# ---------------------------------------------------------------- selection -------------------------------------------------------
def _record_quantities():
    from pta_replicator_amd import _population
    z, k = record()
    mc, dl, hs, fo = _population.cell_quantities(z["vals"], RecordHelpers)
    w = pr.weights(z["weights"], hs ** 2, fo, float(z["T_obs"]))
    return z, k, mc / _population.MSOL_CGS, dl / _population.PC_CGS / 1e6, fo, w


def test_selection_twin_matches_the_reference_record(ph):
    """tests/golden/population.npz with its weights as counts and the helper functions it was recorded with: the selected fo, mc, dl and
    w are the record's bits, in its order; free_spec within 2 n 2^-53 of a long-double sum."""
    z, k, mc, dl, fo, w = _record_quantities()
    cells, count, free, members = pr.select(w, fo, z["fobs"], k)
    assert np.array_equal(fo[cells], z["ret_outlier_fo"])
    assert np.array_equal(mc[cells], z["ret_outlier_mc"])
    assert np.array_equal(dl[cells], z["ret_outlier_dl"])
    assert np.array_equal(w[cells], z["ret_outlier_hs"])
    assert count.tolist() == [4, 4, 4, 4, 4, 2]
    bound = 2 * np.maximum(members, 1) * 2.0 ** -53
    assert np.all(np.abs(z["ret_free_spec"] - free) <= bound * free), (z["ret_free_spec"] - free) / free
    # the order of the record is unambiguous: in no bin does a selected w tie with another selected one or with the loudest cell
    # left out.  (Cells 5 and 17 of the record do tie, at w = 4e-33 far down the rest of bin 0, where the order moves nothing.)
    k_of = np.digitize(fo, z["fobs"]) - 1
    for b in range(len(z["fobs"]) - 1):
        top = np.sort(w[k_of == b])[::-1][:k + 1]
        assert len(np.unique(top)) == len(top), b
    # the header's weight is the twin's, bit for bit
    rows = np.random.default_rng(1).uniform(0, 50, (200, 4)) * [1, 1e-30, 1e-8, 1e8]
    assert all(ph.ph_weight(*map(float, r)) == float(pr.weights(r[0], r[1], r[2], r[3])) for r in rows)


def test_tie_rule_of_the_twin():
    fobs = np.array([1.0, 2.0, 3.0])
    fo = np.array([1.5, 1.5, 1.5, 2.5, 1.5, 0.5])
    cells, count, free, members = pr.select(np.array([2.0, 3.0, 2.0, 0.0, 2.0, 9.0]), fo, fobs, 3)
    assert cells.tolist() == [1, 0, 2] and count.tolist() == [3, 0] and members.tolist() == [4, 1]
    assert float(free[0]) == 2.0 and float(free[1]) == 1e-100


# ---------------------------------------------------------------- tables and interface -------------------------------------------
def test_tables_follow_digitize():
    from pta_replicator_amd import _pop
    vals, number, fobs, T_obs = synthetic([0, 1, 5, 300, 17], lam=(1e-3, 1e8), outside=9)
    number[::11] = 0.0
    tab = _pop.make_tables(vals, number, fobs, T_obs, outlier_per_bin=3)
    k_of = np.digitize(vals[3], fobs) - 1
    inside = (k_of >= 0) & (k_of < 5)
    assert tab["B"] == vals.shape[1] and tab["F"] == 5 and inside.sum() == len(tab["orig"]) == vals.shape[1] - 9
    assert sorted(tab["orig"].tolist()) == np.flatnonzero(inside).tolist()
    assert tab["cell_ptr"].tolist() == np.concatenate([[0], np.cumsum([0, 1, 5, 300, 17])]).tolist()
    for b in range(5):
        sl = slice(tab["cell_ptr"][b], tab["cell_ptr"][b + 1])
        assert np.all(k_of[tab["orig"][sl]] == b)
        reg = _pop.regime(tab["number"][sl])
        assert np.all(np.diff(reg) >= 0)                                    # the regimes of a bin are contiguous
        assert np.all(np.diff(tab["number"][sl])[np.diff(reg) == 0] >= 0)
    assert np.array_equal(tab["number"], number[tab["orig"]]) and np.array_equal(tab["fo"], vals[3][tab["orig"]])
    assert np.array_equal(tab["log10_fo"], np.log10(vals[3])) and tab["log10_mc"].shape == (tab["B"],)
    assert _pop.regime([0.0, 1e-9, 9.999, 10.0, 2.0 ** 20 - 1, 2.0 ** 20, 1e12]).tolist() == [0, 1, 1, 2, 2, 3, 3]
    from pta_replicator_amd import _population
    assert np.array_equal(_population.f_centers(fobs), np.array([(fobs[i + 1] + fobs[i]) / 2 for i in range(5)]))


def test_refusals_before_any_launch():
    vals, number, fobs, T_obs = synthetic([40, 30, 20, 10, 5, 3])
    eng = engine(fobs)
    ok = dict(vals=vals, number=number, fobs=fobs, T_obs=T_obs, outlier_per_bin=3)

    def refused(match, e=None, **kw):
        with pytest.raises(ValueError, match=match):
            (e or eng).set_population(**{**ok, **kw})
    with pytest.raises(ValueError, match="no population"):
        eng.population_theta(4)
    refused("outlier_per_bin", outlier_per_bin=129)
    refused("outlier_per_bin", outlier_per_bin=0)
    refused("outlier_per_bin", outlier_per_bin=2.5)
    refused("finite and >= 0", number=np.where(np.arange(len(number)) == 3, -1.0, number))
    refused("finite and >= 0", number=np.where(np.arange(len(number)) == 3, np.nan, number))
    refused("finite and >= 0", number=np.where(np.arange(len(number)) == 3, np.inf, number))
    refused(r"vals must be \[4, B\]", vals=vals[:3])
    refused(r"number must be \[B\]", number=number[:-1])
    refused("bin edges", fobs=fobs[:1])
    refused("increasing", fobs=fobs[::-1])
    refused("T_obs", T_obs=0.0)
    big = np.arange(1, 67) / T_obs
    refused("at most 64", fobs=big)
    refused("node frequencies", fobs=fobs * 1.001)                        # the userSpec's nodes are not these bins' centres
    refused("node frequencies", fobs=fobs[:-1])
    refused("set_cw", e=engine(fobs, cw=False))
    e = engine(fobs)
    e.set_gwb(-14.5, 13.0 / 3.0)
    refused("userSpec", e=e)
    e = engine(fobs)
    e.set_cw_prior(log10_mc=(8, 9), log10_fgw=(-8.5, -8), log10_dist=(1, 2), n_sources=18)
    refused("set_cw_prior", e=e)
    e = engine(fobs)
    e.set_hyper_prior(gwb_log10_hc=(-16, -14))
    refused("gwb_log10_hc", e=e)
    e = engine(fobs)
    e._td_prepared = True                                                  # what prepare_td() leaves behind
    refused("TD mode", e=e)
    # population_theta checks the configuration again: it may have changed since set_population
    e = engine(fobs)
    e.set_population(**ok)
    with pytest.raises(ValueError, match=r"counts must be \[R, B\]"):
        e.population_theta(4, counts=np.ones((3, len(number))))
    with pytest.raises(ValueError, match="finite and >= 0"):
        e.population_theta(2, counts=-np.ones((2, len(number))))
    e.set_cw_prior(log10_mc=(8, 9), log10_fgw=(-8.5, -8), log10_dist=(1, 2), n_sources=18)
    with pytest.raises(ValueError, match="set_cw_prior"):
        e.population_theta(4)
    e = engine(fobs)
    e.set_population(**ok)
    e._td_prepared = True
    with pytest.raises(ValueError, match="TD mode"):
        e.population_theta(4)
    e = engine(fobs)
    e.set_population(**ok)
    e.set_gwb(None, None, userSpec=user_spec(fobs * 1.01))
    with pytest.raises(ValueError, match="node frequencies"):
        e.population_theta(4)
    # removed again
    e = engine(fobs)
    assert e.set_population(**ok) is e and e._pop is not None
    assert e.set_population(None) is e and e._pop is None
    with pytest.raises(ValueError, match="no prior"):
        e.sample_theta(2)


def test_label_keys_are_skipped_by_theta():
    from pta_replicator_amd import _pop
    th = {"pop_cell": 1, "pop_number": 2, "cw_count": 3}
    assert _pop.strip_labels(th) == {"cw_count": 3} and _pop.strip_labels({"a": 1}) == {"a": 1}
