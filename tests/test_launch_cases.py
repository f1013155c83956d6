"""tests/launch_cases.py against the library's own launch plans: every case reaches the kernel instance it names, and together the
cases reach every instance a launcher can choose.  No GPU: the pta_*_plan entries make no device call."""
import launch_cases as lc


def _plans(launcher):
    return [(c, lc.plan(c["launcher"], *c["sizes"])) for c in lc.ALL_CASES if c["launcher"] == launcher]


def test_every_case_reaches_the_instance_it_names():
    assert len(lc.ALL_CASES) > 150
    for c in lc.ALL_CASES:
        got = lc.plan(c["launcher"], *c["sizes"])
        assert c["expect"] and all(got[k] == v for k, v in c["expect"].items()), (c, got)


def test_os_project_cases_cover_both_tile_counts_of_every_column_count():
    reached = {(p["rw"], p["ct"]) for _, p in _plans("pta_os_project")}
    print("pta_os_project (rw, ct):", sorted(reached))
    assert reached == {(rw, ct) for rw in (1, 2) for ct in (1, 2, 3, 4)}
    # the small launches are the windows the GPU test recomputes
    small = {c["sizes"][2] for c, p in _plans("pta_os_project") if p["rw"] == 1}
    assert {n for R in lc.OS_R for _, n in lc.os_windows(R)} <= small
    counts = lc.os_counts()
    assert len(counts) == lc.OS_P and counts.min() == 1 and sorted(counts)[-5:] == [65, 130, 130, 257, 301]
    lo, n = lc.OS_WINDOW
    assert sum(1 for a in lc.OS_LONG if lo <= a < lo + n) == 4


def test_lnl_apply_cases_cover_every_kt_and_the_grid_point_groups():
    plans = _plans("pta_lnl_apply")
    kts = {p["kt"] for _, p in plans}
    print("pta_lnl_apply kt:", sorted(kts), "g_per:", sorted({p["g_per"] for _, p in plans}))
    assert kts == set(range(1, 9))
    G_of = lambda c: c["sizes"][2]
    assert any(p["g_per"] == 1 for _, p in plans)
    assert any(2 <= p["g_per"] <= 15 and G_of(c) % p["g_per"] != 0 for c, p in plans)          # a short last group
    assert any(p["g_per"] == 16 and G_of(c) % 16 != 0 and p["gz"] == lc.cdiv(G_of(c), 16) for c, p in plans)
    for c in lc.LNL_GROUPS:   # the recomputed grid points hold the whole short last group, the realisations the last of a partial tile
        last = (c["G"] - 1) // c["g_per"] * c["g_per"]
        assert c["G"] % c["g_per"] == 0 or set(range(last, c["G"])) <= set(c["sub_g"])
        assert c["R"] - 1 in c["sub_r"] and 0 in c["sub_g"] and max(c["sub_g"]) < c["G"] and max(c["sub_r"]) < c["R"]
        assert lc.plan("pta_lnl_apply", c["P"], c["K"], len(c["sub_g"]), len(c["sub_r"]))["g_per"] == 1


def test_fstat_project_cases_cover_all_six_tiles():
    reached = {(p["bm"], p["bn"]) for _, p in _plans("pta_fstat_project")}
    print("pta_fstat_project (bm, bn):", sorted(reached))
    assert reached == {(bm, bn) for bm in (64, 128) for bn in (32, 64, 128)}


def test_mix_cases_cover_both_sides_of_512_realisations():
    plans = _plans("pta_gwb_mix_batched")
    ntile = lc.cdiv(lc.MIX_NPTS, lc.MIX_TILE)
    assert ntile > 4
    for P in lc.MIX_P:
        mine = {c["sizes"][1]: p for c, p in plans if c["sizes"][0] == P}
        print(f"pta_gwb_mix_batched P={P}:", mine)
        assert mine[511]["tpw"] == 4 and mine[511]["grid_x"] * 4 > ntile          # the last workgroup leaves its loop before tile 8
        assert mine[512]["tpw"] == ntile and mine[512]["grid_x"] == 1
        assert mine[lc.MIX_SMALL_R]["tpw"] == 4
        assert mine[511]["nta"] == mine[512]["nta"] == lc.cdiv(P, 16)
    assert {p["nta"] for _, p in plans} == {1, 2, 3, 4, 5}


def test_sky_statistic_cases_cover_every_ks_and_the_chunkings():
    for name, rb in lc.SKY_RB.items():
        plans = _plans(name)
        kss = {p["ks"] for _, p in plans}
        chunks = sorted({(p["rchunk"], p["ngz"]) for c, p in plans if c["sizes"][2] > 8})
        print(f"{name}: ks {min(kss)}..{max(kss)} ({len(kss)} values), (rchunk, ngz) of the large launches {chunks}")
        assert kss == set(range(1, 33))
        assert {p["ks"] for c, p in plans if c["sizes"][0] % 4 == 0} and {p["ks"] for c, p in plans if c["sizes"][0] % 4 == 1}
        assert any(p["ngz"] > 1 and p["rchunk"] % rb == 0 for _, p in plans)
        assert any(p["ngz"] > 1 and p["rchunk"] % rb != 0 for _, p in plans)
        assert any(p["ngz"] == 1 and p["rchunk"] == c["sizes"][2] and c["sizes"][2] % rb != 0 for c, p in plans)    # nz = 1
        for c in lc.SKY_CHUNK[name]:   # a recomputed window straddles a chunk boundary, and one ends at R
            p = lc.plan(name, c["P"], c["J"], c["R"], c["S"])
            assert p["rchunk"] == c["rchunk"]
            assert any(lo + n == c["R"] for lo, n in c["windows"])
            assert p["ngz"] == 1 or any(lo // p["rchunk"] != (lo + n - 1) // p["rchunk"] for lo, n in c["windows"])
    assert len(set(lc.SKY_KS_P)) == len(lc.SKY_KS_P) and {lc.cdiv(P, 4) for P in lc.SKY_KS_P} == set(range(1, 33))


def test_tm_project_cases_cover_every_m():
    plans = _plans("pta_tm_project")
    assert {p["m"] for _, p in plans} == set(range(1, 13))
    assert {c["sizes"][2] % 8 for c, _ in plans} >= {0, 1, 7} and {p["grid_y"] for _, p in plans} == {1, 2, 3}
    print("pta_tm_project m:", sorted({p["m"] for _, p in plans}), "R:", lc.TM_R)
