"""A binned binary population per realisation on the MI355X (set_population, pta_pop_draw_select, pta_pop_theta): the drawn counts against
the g++ build of csrc/pta_pop.h, the selection against its NumPy twin over the bin sizes and orders at which the kernel takes another
path, the reference's record through the ABI, the independence of a row from the launch it sits in, the engine's entry points, and
the strain budget of an ensemble."""
import numpy as np
import pytest
import torch

import pop_reference as pr
from pop_cases import FLAG_CAP, RecordHelpers, build_host, engine, host_poisson, record, synthetic

pytestmark = pytest.mark.gpu

SEED = 20260131
CHUNK = 1024   # PTA_POP_CHUNK
LN10 = float(np.log(10.0))


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("pop_gpu"))


def _run(tab, R, r0=0, counts=None, step=None, seed=SEED):
    """population_run over fresh device tables -> {key: NumPy array}"""
    from pta_replicator_amd import engine_terms as et
    out = et.population_run(et.population_device_tables(tab), seed, R, r0, counts=counts, raw=True, step=step)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---------------------------------------------------------------- draws ------------------------------------------------------------
def _all_regimes():
    """one bin: 1 cell without a rate, 63 of the inversion regime, 64 of PTRS, 65 of the normal regime, the boundaries 10 and 2^20
    among them, in shuffled cell order"""
    rng = np.random.default_rng(2)
    lam = np.concatenate([[0.0], np.r_[10 ** rng.uniform(-6, 0.99, 60), 1e-6, 9.999, np.nextafter(10.0, 0)],
                          np.r_[10 ** rng.uniform(1, 6, 60), 10.0, 10.001, 37.5, float((1 << 20) - 1)],
                          np.r_[10 ** rng.uniform(6.03, 9, 63), float(1 << 20), 1e9]])
    lam = lam[rng.permutation(len(lam))]
    vals, _, _, T_obs = synthetic([len(lam)], outside=0)
    fobs = np.array([1.0, 2.0]) / T_obs
    return vals, lam, fobs, T_obs


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("r0", [0, (1 << 32) + 3])
def test_drawn_counts_match_the_host_build(ph, R, r0):
    from pta_replicator_amd import _pop
    vals, lam, fobs, T_obs = _all_regimes()
    assert np.bincount(_pop.regime(lam)).tolist() == [1, 63, 64, 65]
    got = _run(_pop.make_tables(vals, lam, fobs, T_obs, outlier_per_bin=4), R, r0)["pop_counts"]
    B = len(lam)
    rho = np.repeat(np.uint64(r0) + np.arange(R, dtype=np.uint64), B)
    cell, lams = np.tile(np.arange(B, dtype=np.uint32), R), np.tile(lam, R)
    want, _ = host_poisson(ph, SEED, rho, cell, lams)
    _, flag, _ = pr.poisson(SEED, rho, cell, lams)
    bad = (got.ravel() != want) & ~flag
    print(f"R = {R}, r0 = {r0}: flagged {flag.sum()} of {len(flag)}, mismatches among the rest {bad.sum()}")
    assert flag.mean() <= FLAG_CAP
    assert not bad.any(), (lams[bad], got.ravel()[bad], want[bad])


# ---------------------------------------------------------------- selection --------------------------------------------------------
def _uniform_bins(sizes, T_obs=10 * 365.25 * 86400.0):
    """every cell of a bin the same binary, all rates 1: w is an increasing function of the count alone and the tables keep a bin's
    cells in cell order"""
    F = len(sizes)
    fobs = np.arange(1, F + 2) / T_obs
    fo = np.concatenate([np.full(n, 0.5 * (fobs[b] + fobs[b + 1])) for b, n in enumerate(sizes)])
    B = len(fo)
    vals = np.array([np.full(B, 3e9 * 1.988409870698051e33), np.full(B, 0.7), np.full(B, 0.3), fo])
    return vals, np.ones(B), fobs, T_obs


@pytest.mark.parametrize("k", [1, 4, 100, 128])
def test_selection_matches_the_twin(k):
    from pta_replicator_amd import _pop, _population
    sizes = [0, 1, max(k - 1, 0), k, k + 1, 255, 256, 257, CHUNK + 1, 3 * CHUNK + 5]
    vals, number, fobs, T_obs = _uniform_bins(sizes)
    tab = _pop.make_tables(vals, number, fobs, T_obs, outlier_per_bin=k)
    assert np.array_equal(tab["orig"], np.arange(len(number)))
    B, F = len(number), len(sizes)
    rng = np.random.default_rng(k)
    pos = np.arange(B, dtype=np.float64)
    few = np.zeros(B)
    few[rng.permutation(B)[:max(1, (k // 2) * F)]] = rng.integers(1, 50, max(1, (k // 2) * F))
    counts = np.stack([1.0 + pos,                                   # w ascending in cell order: every chunk forces a prune
                       float(B) - pos,                              # descending: the first k of every bin, nothing pushed after them
                       np.full(B, 7.0),                             # all equal and positive: the tie rule
                       np.zeros(B),                                 # all zero
                       few,                                         # fewer than k positive in most bins
                       rng.integers(0, 1000, B).astype(np.float64)])  # ties and zeros at random
    got = _run(tab, len(counts), counts=counts)
    _, _, hs, fo = _population.cell_quantities(vals)
    S = F * k
    for r, row in enumerate(counts):
        w = pr.weights(row, hs ** 2, fo, T_obs)
        cells, count, free, members = pr.select(w, fo, fobs, k)
        n = len(cells)
        assert got["cw_count"][r] == n and np.array_equal(got["pop_sel_count"][r], count), (r, got["pop_sel_count"][r], count)
        assert np.array_equal(got["pop_cell"][r, :n], cells) and np.all(got["pop_cell"][r, n:] == -1), r
        assert np.array_equal(got["pop_number"][r, :n], row[cells]) and np.all(np.isnan(got["pop_number"][r, n:])), r
        sel_w = np.concatenate([got["pop_sel_w"][r, b, :count[b]] for b in range(F)])
        assert np.array_equal(sel_w, w[cells]), r
        for key, tab_key in (("cw_log10_mc", "log10_mc"), ("cw_log10_fgw", "log10_fo"), ("cw_log10_dist", "log10_dl")):
            assert np.array_equal(got[key][r, :n], tab[tab_key][cells]) and np.all(np.isnan(got[key][r, n:])), (r, key)
        nb = np.maximum(members, 1)
        err = np.abs(got["pop_free_spec"][r].astype(np.longdouble) - free) / free
        assert np.all(err <= 2 * nb * 2.0 ** -53), (r, err.astype(float), nb)
        hc = (0.5 * np.log10(free)).astype(np.float64)
        assert np.all(np.abs(got["gwb_log10_hc"][r] - hc) <= 4 * 2.0 ** -53 * np.abs(hc) + nb * 2.0 ** -52 / LN10), r
    assert not got["cw_count"][3] and np.all(got["pop_free_spec"][3] == 1e-100) and np.all(np.abs(got["gwb_log10_hc"][3] + 50.0) <= 4 * 2.0 ** -53 * 50)
    assert np.all(got["pop_free_spec"][:, 0] == 1e-100)             # the empty bin


def test_reference_record_through_the_abi():
    """tests/golden/population.npz, its weights as the counts, the helper functions it was recorded with: the device selects the record's
    sources with the record's bits"""
    from pta_replicator_amd import _pop, _population
    z, k = record()
    tab = _pop.make_tables(z["vals"], np.ones(z["vals"].shape[1]), z["fobs"], float(z["T_obs"]), outlier_per_bin=k, population=RecordHelpers)
    got = _run(tab, 1, counts=z["weights"][None, :])
    n = len(z["ret_outlier_hs"])
    count = got["pop_sel_count"][0]
    assert got["cw_count"][0] == n and count.tolist() == [4, 4, 4, 4, 4, 2]
    assert np.array_equal(np.concatenate([got["pop_sel_w"][0, b, :count[b]] for b in range(6)]), z["ret_outlier_hs"])
    assert np.array_equal(got["cw_log10_fgw"][0, :n], np.log10(z["ret_outlier_fo"]))
    assert np.array_equal(got["cw_log10_mc"][0, :n], np.log10(z["ret_outlier_mc"]))
    assert np.array_equal(got["cw_log10_dist"][0, :n], np.log10(z["ret_outlier_dl"]))
    assert np.array_equal(got["pop_number"][0, :n], z["weights"][got["pop_cell"][0, :n]])
    _, _, hs, fo = _population.cell_quantities(z["vals"], RecordHelpers)
    _, _, free, members = pr.select(pr.weights(z["weights"], hs ** 2, fo, float(z["T_obs"])), fo, z["fobs"], k)   # the long-double sum
    assert np.all(np.abs(got["pop_free_spec"][0] - free) <= 2 * members * 2.0 ** -53 * free)
    hc = (0.5 * np.log10(free)).astype(np.float64)
    assert np.all(np.abs(got["gwb_log10_hc"][0] - hc) <= 4 * 2.0 ** -53 * np.abs(hc) + members * 2.0 ** -52 / LN10)


# ---------------------------------------------------------------- engine -----------------------------------------------------------
SIZES = (900, 700, 500, 300, 150, 2)
K = 3


@pytest.fixture(scope="module")
def pop():
    vals, number, fobs, T_obs = synthetic(list(SIZES), seed=8, lam=(1e-3, 3e3), outside=11)
    number[::53] = 0.0
    number[5::301] = 3e6                      # the normal regime
    return vals, number, fobs, T_obs


@pytest.fixture(scope="module")
def eng(pop):
    vals, number, fobs, T_obs = pop
    return engine(fobs).set_population(vals, number, fobs, T_obs, outlier_per_bin=K)


def _np(theta):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in theta.items()}


@pytest.fixture(scope="module")
def singles(eng):
    """population_theta(1, r0 + r) for r < 33, computed once"""
    r0 = (1 << 33) + 5
    return r0, [_np(eng.population_theta(1, r0 + r)) for r in range(33)]


@pytest.mark.parametrize("R", [1, 7, 33])
def test_a_row_does_not_depend_on_its_launch(eng, singles, R):
    r0, one = singles
    S = len(SIZES) * K
    per_real = 20 * S + 12 * len(SIZES)
    for ws in (8 << 30, 3 * per_real, 5 * per_real + 7):   # one batch; batches of 3; batches of 5
        eng.workspace_bytes = ws
        try:
            got = _np(eng.population_theta(R, r0))
        finally:
            eng.workspace_bytes = 8 << 30
        assert set(got) == set(one[0]) and got["pop_cell"].shape == (R, S) and got["cw_count"].dtype == np.int32
        for r in range(R):
            for key, v in got.items():
                assert _same(v[r:r + 1], one[r][key]), (ws, r, key)
    assert one[0]["cw_count"][0] > 0 and not _same(one[0]["pop_number"], one[1]["pop_number"])


def test_table_order_does_not_matter(eng, pop):
    """A drawn count is keyed by the caller's cell index, so a permuted population is another sample; what must not matter is how the
    tables order the cells.  With the counts of the first run handed to a permuted copy of the population the rows are the same after
    mapping the cell indices."""
    vals, number, fobs, T_obs = pop
    R, r0 = 7, 3
    torch.cuda.synchronize()
    a = {k: v.cpu().numpy() for k, v in eng.population_theta(R, r0, raw=True).items()}
    counts = np.nan_to_num(a["pop_counts"], nan=0.0)
    perm = np.random.default_rng(4).permutation(len(number))
    other = engine(fobs).set_population(vals[:, perm], number[perm] * 0.5 + 1.0, fobs, T_obs, outlier_per_bin=K)   # other rates: another table order
    b = _np(other.population_theta(R, r0, counts=counts[:, perm]))
    with_counts = _np(eng.population_theta(R, r0, counts=counts))
    for key in with_counts:
        assert _same(with_counts[key], a[key]), key                # explicit counts = the drawn ones
        if key == "pop_cell":
            assert np.array_equal(np.where(b[key] >= 0, perm[np.maximum(b[key], 0)], -1), a[key])
        elif key == "gwb_log10_hc":   # the rest is summed in table order: two sums of n non-negative terms, each within its bound
            assert np.all(np.abs(b[key] - a[key]) <= 2 * (4 * 2.0 ** -53 * np.abs(a[key]) + max(SIZES) * 2.0 ** -52 / LN10))
        else:
            assert _same(b[key], a[key]), key


def test_engine_entry_points(eng, pop):
    vals, number, fobs, T_obs = pop
    R, r0 = 6, 17
    out, labels = eng.generate_sampled(R, r0)
    want = eng.population_theta(R, r0)
    assert set(labels) == set(want) and "pop_cell" in labels and "cw_cos_inc" in labels
    for key in want:
        assert _same(labels[key].cpu().numpy(), want[key].cpu().numpy()), key
    assert int(labels["cw_count"].min()) > 0 and torch.isfinite(out).all()
    assert torch.equal(eng.generate(R, r0, theta=labels), out)
    per = eng.generate_per_signal(R, r0, theta=labels)
    assert torch.equal(per["total"], out)
    plain = engine(fobs)                                            # no population: the catalogue term of the same labels
    cw_only = {k: v for k, v in labels.items() if k.startswith("cw_")}
    assert torch.equal(plain.generate_per_signal(R, r0, theta=cw_only)["cw"], per["cw"]) and float(per["cw"].abs().max()) > 0
    # the orientation labels are the catalogue's own draw, source s from stream (8, s)
    plain.set_cw_prior(log10_mc=(8.0, 9.0), log10_fgw=(-8.5, -8.0), log10_dist=(1.0, 2.0), n_sources=len(SIZES) * K)
    drawn = plain.sample_theta(R, r0)
    for key in ("cw_cos_gwtheta", "cw_gwphi", "cw_phase0", "cw_psi", "cw_cos_inc"):
        assert torch.equal(drawn[key], labels[key]), key
    # an engine without the call, or with it taken back, runs what it ran
    base = engine(fobs).generate(R, r0)
    undone = engine(fobs).set_population(vals, number, fobs, T_obs, outlier_per_bin=K).set_population(None)
    assert torch.equal(undone.generate(R, r0), base) and torch.equal(eng.generate(R, r0), base)


def test_strain_budget_of_an_ensemble():
    """R = 512 on 2000 cells: the mean over realisations of sum_k (free_spec - 1e-100 + sum of the selected w) is sum_b number_b c_b,
    c_b = hs2_b fo_b T_obs, within 5 standard errors; the variance of one realisation is sum_b number_b c_b^2, the normal regime included."""
    from pta_replicator_amd import _pop, _population
    vals, number, fobs, T_obs = synthetic([700, 500, 400, 250, 100, 50], seed=21, lam=(1e-3, 1e4), outside=0)
    number[3::211] = 5e6
    R = 512
    got = _run(_pop.make_tables(vals, number, fobs, T_obs, outlier_per_bin=5), R, r0=1000)
    _, _, hs, fo = _population.cell_quantities(vals)
    c = hs ** 2 * fo * T_obs
    total = (got["pop_free_spec"] - 1e-100).sum(axis=1) + got["pop_sel_w"].sum(axis=(1, 2))
    mean, se = float(np.sum(number * c)), float(np.sqrt(np.sum(number * c ** 2) / R))
    print(f"budget: (mean - expected) / se = {(total.mean() - mean) / se:+.2f}; sample sd / expected sd = {total.std(ddof=1) / (se * np.sqrt(R)):.3f}")
    assert abs(total.mean() - mean) <= 5 * se
    assert np.all(got["pop_counts"] >= 0) and np.all(got["pop_counts"] == np.floor(got["pop_counts"]))
