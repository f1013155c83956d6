"""Hand-built plans for the fused synthesis pass: the operands tests/test_synth_reference_host.py (CPU) and
tests/test_gpu_synth_direct.py (MI355X) evaluate - test infrastructure, not product code.

Every operand is O(1) - design matrix, coefficients, grid series and deterministic term normal (with exact zeros among the first
two), noise amplitudes uniform in (0.5, 2) - so that every term is visible on its own against a bound near 1e-14: a term that is
wrong, misplaced or drawn from the wrong counter is wrong by O(1)."""
import numpy as np

TILE, EPMAX = 256, 132   # PTA_ENGINE_TILE, PTA_ENGINE_EPMAX (asserted against _lib by the GPU test)

# TOAs per pulsar: a tile that ends one short of, at and one past every wave boundary (64) and, the counts being odd and even, every
# boundary of a lane's pair of adjacent TOAs; full tiles followed by a short one (543 = 2 x 256 + 31) and by nothing (768)
COUNTS = (1, 2, 63, 64, 65, 129, 192, 193, 255, 256, 257, 543, 768)
# every residue of the group of four bins (K even: 0, 2) and of the rotation's trip of twelve (2, 4, 6, 10, 0), at one, two and five trips
KS = (2, 4, 6, 10, 12, 14, 22, 24, 26, 58, 60, 62)
RS = (1, 15, 16, 17, 33)
SEEDS = ((7, 0), (0x9E3779B97F4A7C15, 2 ** 32 - 3), (0xDEADBEEF12345678, 2 ** 40 + 1))
PLANS = ("all", "no_rn", "no_gw", "no_wn", "no_ec", "no_det", "ec_only", "rn_only")
SUBPLANS = (1, 7, 9)     # tiles of a strict subset of the tile table, not in pulsar order: 2, 14, 18 work items at R = 17
IDX_OFFSET = 2_000_000_000


def tiles_of(counts):
    off = np.concatenate([[0], np.cumsum(counts)])
    t = [(a, int(off[a]) + s0, min(TILE, int(n) - s0)) for a, n in enumerate(counts) for s0 in range(0, int(n), TILE)]
    return off, np.array(t, dtype=np.int32).reshape(-1, 3)


def _epochs(rng, kind, a, n):
    """epoch_of for a pulsar of n TOAs (B.2 of the issue this file was written for):
    i    epochs of 1 to 3 adjacent TOAs, numbered consecutively from a & 1 - a tile's first epoch is odd in one pulsar, even in another
    ii   numbers with gaps: every tile of two or more TOAs touches exactly EPMAX pairs
    iii  the same with EPMAX + 1 pairs: not staged, the deviates are evaluated per TOA
    iv   as i, in shuffled order inside each tile"""
    e = np.zeros(n, dtype=np.int64)
    if kind in ("i", "iv"):
        i, nxt = 0, a & 1
        while i < n:
            m = int(rng.integers(1, 4))
            e[i:i + m] = nxt
            i, nxt = i + m, nxt + 1
        if kind == "iv":
            for s0 in range(0, n, TILE):
                rng.shuffle(e[s0:s0 + TILE])
        return e
    npair = EPMAX if kind == "ii" else EPMAX + 1
    base = a & 1
    for s0 in range(0, n, TILE):
        c = min(TILE, n - s0)
        last = 2 * ((base >> 1) + npair - 1) + int(rng.integers(0, 2))
        if c == 1:
            e[s0] = base
        else:
            mid = np.sort(rng.integers(base, last + 1, c - 2))
            e[s0:s0 + c] = np.concatenate([[base], mid, [last]])
        base = int(e[s0 + c - 1]) + 1 + ((a >> 1) & 1)
    return e


def ecorr_tile_tables(tiles, off, epoch_of):
    """tile_ep0 / tile_epn as pta_replicator_amd/engine.py's prepare() sets them"""
    ep0, epn = [], []
    for a, s, c in tiles:
        e = epoch_of[s:s + c]
        p0, p1 = int(e.min()) >> 1, int(e.max()) >> 1
        ep0.append(p0)
        epn.append(p1 - p0 + 1 if p1 - p0 + 1 <= EPMAX else 0)
    return np.array(ep0, dtype=np.int32), np.array(epn, dtype=np.int32)


def make_case(K=60, R=17, seed=7, r0=0, plan="all", ecorr="i", npts=601, single=False, perm=False, fast=False, subplan=None,
              counts=COUNTS):
    """a plan (dict of NumPy arrays, see synth_reference) plus the call's scalars, reproducible from the arguments alone"""
    rng = np.random.default_rng([K, R, r0 % 1000, PLANS.index(plan), "i ii iii iv".split().index(ecorr), npts, int(single), int(perm),
                                 subplan or 0, len(counts)])
    P, n = len(counts), int(sum(counts))
    off, tiles = tiles_of(counts)
    has = dict(rn=plan not in ("no_rn", "ec_only"), gw=plan not in ("no_gw", "ec_only", "rn_only"),
               wn=plan not in ("no_wn", "ec_only", "rn_only"), ec=plan not in ("no_ec", "rn_only"),
               det=plan not in ("no_det", "ec_only", "rn_only"))
    pa = dict(n_toa=n, n_psr=P, rn_k=K if has["rn"] else 0, gw_npts=npts if has["gw"] else 0)
    idx = np.concatenate([np.arange(c) for c in counts])
    if perm:   # the contract only says "pair index": any value will do in the two-deviate mode
        idx = np.concatenate([rng.permutation(c) for c in counts]) + IDX_OFFSET
    pa["idx_in_psr"] = idx.astype(np.int32)
    if has["rn"]:
        Ft = rng.standard_normal((K, n))
        Ft[rng.random((K, n)) < 0.05] = 0.0
        cf = rng.standard_normal((R, P, K))
        cf[rng.random((R, P, K)) < 0.05] = 0.0
        pa["Ft"], pa["rn_coef"] = Ft, cf
        pa["Ft_beyond"] = rng.standard_normal((3, n))   # host only: what a read past bin K - 1 would find (never on the device)
    if has["gw"]:
        pa["gw_G"] = rng.standard_normal((R, P, npts))
        j = rng.integers(0, npts - 1, n)
        w = rng.random(n)
        for a, s, c in tiles:      # the first and the last bracket, weights exactly 0 and 1, at both ends of every tile
            j[s], j[s + c - 1] = npts - 2, 0
            w[s], w[s + c - 1] = 1.0, 0.0
        j[rng.random(n) < 0.1] = npts - 2
        pa["gw_jlo"], pa["gw_w"] = j.astype(np.int32), w
    if has["wn"]:
        if single:
            pa["wn_c"] = rng.uniform(0.5, 2.0, n)
        else:
            pa["wn_a"], pa["wn_b"] = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    epoch_of = np.zeros(n, dtype=np.int64)
    if has["ec"]:
        epoch_of = np.concatenate([_epochs(rng, ecorr, a, int(c)) for a, c in enumerate(counts)])
        ec = rng.uniform(0.5, 2.0, n)
        if ecorr == "iii":
            ec[rng.random(n) < 1.0 / 3.0] = 0.0
        pa["epoch_of"], pa["ecorr_toa"] = epoch_of.astype(np.int32), ec
        ep0, epn = ecorr_tile_tables(tiles, off, epoch_of)
        full = tiles[:, 2] == TILE
        if ecorr == "ii":
            assert np.all(epn[full] == EPMAX)
        if ecorr == "iii":
            assert np.all(epn[tiles[:, 2] > 1] == 0)
    else:
        ep0 = epn = np.zeros(len(tiles), dtype=np.int32)
    if has["det"]:
        pa["det"] = rng.standard_normal(n)
    if fast:
        # the fp32 transform's bound, 2e-5 x the noise amplitudes, would hide the other terms everywhere: one TOA in ten has no noise,
        # and there the bound is the fp64 one
        quiet = rng.random(n) < 0.1
        quiet[tiles[:, 1]] = True      # (a tile's first TOA among them: where a store past the previous tile's last TOA lands)
        for k in ("wn_a", "wn_b", "wn_c", "ecorr_toa"):
            if k in pa:
                pa[k][quiet] = 0.0
    if subplan is not None:
        keep = rng.permutation(len(tiles))[:subplan]
        if subplan > 1 and np.all(np.diff(keep) > 0):
            keep = keep[::-1]
        tiles, ep0, epn = tiles[keep], ep0[keep], epn[keep]
    pa["tile_psr"], pa["tile_start"], pa["tile_count"] = (np.ascontiguousarray(tiles[:, k]) for k in range(3))
    pa["tile_ep0"], pa["tile_epn"] = ep0, epn
    return dict(pa=pa, seed=seed, r0=r0, R=R, single=single, fast=fast, K=K, plan=plan, ecorr=ecorr, npts=npts, perm=perm,
                subplan=subplan)


def _id(kw):
    return "-".join(f"{k}{v:#x}" if k in ("seed", "r0") else f"{k}{v}" for k, v in kw.items()) or "default"


# B.1: the full K list at R = 17 with everything; the full R and (seed, r0) lists at K = 58, 60; the plans and sub-plans at K = 60, R = 17
CASES_K = [dict(K=K) for K in KS]
CASES_BATCH = [dict(K=K, R=R, seed=s, r0=r0) for K in (58, 60) for R in RS for s, r0 in SEEDS]
CASES_PLAN = [dict(plan=p) for p in PLANS[1:]] + [dict(subplan=m, seed=SEEDS[1][0], r0=SEEDS[1][1]) for m in SUBPLANS]
# B.2: the ECORR tables (i is every other case's); K = 58 for iii so that the per-TOA path also meets the tail loop
CASES_ECORR = [dict(ecorr="ii"), dict(ecorr="iii", K=58, seed=SEEDS[2][0], r0=SEEDS[2][1]), dict(ecorr="iv"),
               dict(ecorr="iii", plan="ec_only")]
# B.3: GWB grids of 2, 3 (odd: the pair of bracket samples is then only 8-byte aligned in every other row) and 601 samples; the
# single-deviate white noise; arbitrary pair indices; the fp32 Gaussian transform
CASES_MODES = [dict(npts=2), dict(npts=3), dict(npts=3, plan="no_rn", R=33), dict(single=True), dict(single=True, K=58, R=33),
               dict(single=True, ecorr="iii"), dict(perm=True, seed=SEEDS[1][0], r0=SEEDS[1][1]), dict(fast=True),
               dict(fast=True, single=True, K=58)]
GROUPS = {"B1_K": CASES_K, "B1_batch": CASES_BATCH, "B1_plan": CASES_PLAN, "B2_ecorr": CASES_ECORR, "B3_modes": CASES_MODES}
ALL = [(g, kw) for g, cs in GROUPS.items() for kw in cs]
IDS = [f"{g}-{_id(kw)}" for g, kw in ALL]
