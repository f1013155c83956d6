"""tests/gemm_cases.py against pta_dgemm_plan: every call of every case reaches the kernel instance it names, and together the cases
reach all nine instances, every lower mode each instance has, both sides of each threshold, every vec condition failing alone, the
slab counts with and without a K tail, the tile edges and every caller's form.  No GPU: the query makes no device call."""
import numpy as np

import gemm_cases as gc
import gemm_reference as gr


def _calls():
    return [(case, c, gc.plan(c)) for case in gc.CASES for c in case["calls"]]


def test_names_match_the_library():
    from pta_replicator_amd import _lib
    assert gc.DGEMM_KERNELS == _lib.DGEMM_KERNELS and gc.DGEMM_LOWER == _lib.DGEMM_LOWER
    assert len(set(gc.DGEMM_KERNELS)) == 9
    names = [c["name"] for c in gc.CASES]
    assert len(set(names)) == len(names)


def test_every_case_reaches_the_instance_it_names():
    assert len(gc.CASES) > 120
    for case, c, got in _calls():
        assert "kernel" in c["expect"] and all(got[k] == v for k, v in c["expect"].items()), (case["name"], c["expect"], got)
        assert c["alpha"] in gc.ALPHAS and c["beta"] in gc.BETAS, case["name"]          # powers of two: the exact test's premise
        assert max(c["M"], c["N"]) <= 520 and (c["K"] <= 130 or case["deep"]), case["name"]
    assert sum(case["deep"] for case in gc.CASES) == 1


def test_all_nine_instances_and_their_lower_modes():
    reached = {}
    for case, c, p in _calls():
        reached.setdefault(p["kernel"], set()).add(p["lower_mode"])
    print({k: sorted(v) for k, v in reached.items()})
    assert set(reached) == set(gc.DGEMM_KERNELS)
    for k in (gc.M128_N, gc.M128_T, gc.M128_TV, gc.GLDS_E0, gc.GLDS_E1):
        assert {gc.L_NONE, gc.L_GRID2D, gc.L_TRIANGLE} <= reached[k], k
    for k in (gc.GLDS_E0, gc.GLDS_E1):
        assert gc.L_TRAPEZOID in reached[k], k
    for k in (gc.VALU_N, gc.VALU_T, gc.MFMA_N, gc.MFMA_T):
        assert reached[k] == {gc.L_NONE, gc.L_GRID2D}, k
    # the 2-D early exit on a 128-tile kernel with M < N: tiles strictly above the diagonal exist
    assert any(p["tile"] == 128 and p["lower_mode"] == gc.L_GRID2D and c["M"] < c["N"] and p["grid_x"] > p["grid_y"] for _, c, p in _calls())
    # beta = 0 (NaN in C) and beta != 0 on every instance, batches on every instance
    for k in gc.DGEMM_KERNELS:
        mine = [c for _, c, p in _calls() if p["kernel"] == k]
        assert any(c["beta"] == 0.0 for c in mine) and any(c["beta"] != 0.0 for c in mine), k
        assert any(c["batch"] > 1 for c in mine), k
        assert {c["alpha"] for c in mine} >= {1.0, -1.0} and len({c["beta"] for c in mine}) >= 3, k


def test_each_threshold_from_both_sides():
    for algo, big in ((1, gc.M128_TV), (2, gc.GLDS_E0)):
        got = {(c["M"], c["N"], c["K"]): p["kernel"] for _, c, p in _calls() if c["algo"] == algo and c["transB"] and (c["M"], c["N"], c["K"]) in gc.THRESHOLDS}
        assert got == {s: (big if at else gc.MFMA_T) for s, at in gc.THRESHOLDS.items()}, (algo, got)
    assert {(256, 128, 32), (255, 128, 32), (256, 127, 32), (256, 128, 31)} <= set(gc.THRESHOLDS)


def test_each_vec_condition_fails_alone():
    M, N, K = gc.VEC_SHAPE
    ok = dict(transB=1, M=M, N=N, K=K, lda=K + 22, ska=1, ldb=K + 6, sA=gc.even(M * (K + 22)), sB=gc.even(N * (K + 6)), offA=0, offB=0)
    for algo, vec_kernel in ((1, gc.M128_TV), (2, gc.GLDS_E0)):
        mine = [(case["name"], c, p) for case, c, p in _calls() if case["name"].startswith("vec") and c["algo"] == algo]
        met = [p for n, c, p in mine if "all met" in n]
        assert len(met) == 1 and met[0]["kernel"] == vec_kernel
        seen = set()
        for name, c, p in mine:
            if "all met" in name:
                continue
            a = gc.plan_args(c)
            now = dict(transB=a[0], M=a[1], N=a[2], K=a[3], lda=a[4], ska=a[5], ldb=a[6], sA=a[7], sB=a[8], offA=a[9], offB=a[10])
            diff = {k for k in ok if now[k] != ok[k]}
            if "ska" in diff:
                diff -= {"lda", "sA"}       # the rows of an interleaved operand are twice as long; lda and strideA stay even
                assert now["lda"] % 2 == 0 and now["sA"] % 2 == 0
            for ld, st in (("lda", "sA"), ("ldb", "sB")):
                if ld in diff and st in diff:   # the batch stride follows the leading dimension and stays even
                    diff -= {st}
                    assert now[st] % 2 == 0
            assert len(diff) == 1, (name, diff)
            assert p["kernel"] == gc.M128_T, (name, p)
            seen |= diff
        assert seen == {"ska", "K", "lda", "ldb", "sA", "sB", "offA", "offB"}, (algo, seen)
    for k in ("lda", "ldb", "sA", "sB"):
        assert ok[k] % 2 == 0


def test_slab_counts_with_and_without_a_tail():
    for kern in gc.TILE128:
        Ks = {c["K"] for _, c, p in _calls() if p["kernel"] == kern}
        assert set(gc.SLAB_K_EVEN + gc.SLAB_K_QUAD) <= Ks, (kern, sorted(Ks))
        if kern in (gc.M128_N, gc.M128_T):
            assert set(gc.SLAB_K_ODD) <= Ks, kern
    # (slabs, tail): the last slab sits in buffer 1, 0, 1 without a tail and in 0, 1 with one
    assert {(gc.cdiv(K, 16), K % 16 != 0) for K in gc.SLAB_K_EVEN} == {(2, False), (3, False), (4, False), (3, True), (4, True)}
    assert {(gc.cdiv(K, 16), K % 16 != 0) for K in gc.SLAB_K_ODD} == {(3, True)}
    assert {K % 16 for K in gc.SLAB_K_EVEN + gc.SLAB_K_ODD} >= {0, 1, 2, 14, 15} and {K % 16 for K in gc.SLAB_K_QUAD} == {4, 8, 12}


def test_tile_edges():
    for kern in (gc.MFMA_N, gc.MFMA_T):
        MN = {(c["M"], c["N"]) for _, c, p in _calls() if p["kernel"] == kern}
        assert {m for m, _ in MN} >= {63, 64, 65, 129} and {n for _, n in MN} >= {63, 64, 65, 127, 129}, kern
    for kern in gc.TILE128:
        MN = {(c["M"], c["N"]) for _, c, p in _calls() if p["kernel"] == kern}
        assert {m for m, _ in MN} >= {256, 257, 300, 383, 385} and {n for _, n in MN} >= {128, 129, 257, 300}, kern
        assert any(m % 128 == 1 for m, _ in MN) and any(n % 128 == 1 for _, n in MN), kern        # a last tile of one row, of one column
    assert {c["N"] for _, c, p in _calls() if p["tile"] == 64} >= {127}                             # 127 columns: below the threshold


def test_callers_forms():
    by = {case["name"]: case for case in gc.CASES}
    for name, kern, mode in (("TtT 37x37x40", gc.MFMA_N, gc.L_GRID2D), ("TtT 257x257x34", gc.M128_N, gc.L_TRIANGLE),
                             ("TtT 130x130x6002 (the production depth)", gc.MFMA_N, gc.L_GRID2D)):
        c, = by[name]["calls"]
        p = gc.plan(c)
        assert (p["kernel"], p["lower_mode"]) == (kern, mode) and c["A"]["ld"] == 1 and c["A"]["sk"] == c["B"]["ld"] and c["algo"] == 1
        assert c["A"]["reg"] == c["B"]["reg"] and c["A"]["off"] == c["B"]["off"] and c["beta"] == 0.0 and c["lower"] == 1
    assert by["TtT 130x130x6002 (the production depth)"]["deep"]
    for case in (v for k, v in by.items() if k.startswith("idft")):
        a, b = case["calls"]
        assert (a["A"]["off"], b["A"]["off"], a["A"]["sk"], b["A"]["sk"]) == (2, 3, 2, 2) and (a["beta"], b["beta"]) == (0.0, 1.0)
        assert a["C"] == b["C"] and a["transB"] == 0 and b["B"]["off"] == a["K"] * a["B"]["ld"]
    mixes = [v["calls"][0] for k, v in by.items() if k.startswith("mix")]
    assert {(c["K"], c["algo"], c["A"]["stride"] == 0) for c in mixes} == {(P, a, s) for P in (3, 17, 68) for a in (0, 1) for s in (False, True)}
    assert all(c["batch"] == 3 and c["transB"] == 0 and c["M"] == c["K"] for c in mixes)
    a, b = by["clnl j0=64, blocks of 64 and 5"]["calls"]
    for c in (a, b):
        assert (c["alpha"], c["beta"], c["batch"], c["transB"]) == (-1.0, 1.0, 3, 0) and c["B"]["reg"] == c["C"]["reg"]
        assert c["C"]["off"] == c["K"] * c["B"]["ld"] and c["B"]["off"] == 0                      # C = the rows right behind B's
    assert (a["M"], b["M"]) == (64, 5) and b["K"] == a["K"] + a["M"] and "B" not in b["fill"]
    syrks = [v["calls"][0] for k, v in by.items() if k.startswith("syrk")]
    assert {(c["M"], c["N"], c["K"], c["algo"]) for c in syrks} == {s + (a,) for s in ((300, 300, 46), (300, 130, 46), (515, 257, 64)) for a in (1, 2, 3)}
    for c in syrks:
        assert c["A"]["off"] == c["B"]["off"] and c["C"]["off"] == c["A"]["off"] + c["K"] and c["A"]["ld"] == c["C"]["ld"] and c["batch"] == 2
        assert len({c[k]["reg"] for k in "ABC"}) == 1 and c["lower"] == 1
    t = by["trmm 17x130x130"]["calls"][0]
    assert (t["transB"], t["M"], t["N"], t["K"]) == (1, 17, 130, 130)


def test_slabs_are_nan_outside_the_operands_and_guarded():
    """the builder: one allocation, >= 128 guard rows of the widest pitch at both ends and between the buffers, NaN wherever no operand lies,
    the other plane of an interleaved operand NaN, C NaN when beta = 0"""
    for case in gc.CASES:
        if case["deep"]:
            continue
        for kind in ("exact", "bound"):
            s = gr.Slab(case, kind)
            for i, c in enumerate(case["calls"]):
                pre = s.prepare(i)
                ix = s.idx(i)
                used = np.zeros(s.size, bool)
                for k in "ABC":
                    used[ix[k]] = True
                if i == 0:
                    assert np.all(np.isnan(pre[~used])), case["name"]
                for k in "ABC":                   # 128 rows of the operand's own pitch before and behind it are inside the allocation
                    pitch = max(c[k]["ld"], c[k]["sk"])
                    assert ix[k].min() >= 128 * pitch and s.size - 1 - ix[k].max() >= 128 * pitch, (case["name"], k)
                for k in "AB":
                    assert np.all(np.isfinite(pre[ix[k]])), (case["name"], k)
                    assert (ix[k].ravel()[0] % 2 == 0) == (c[k]["off"] % 2 == 0)            # alignment follows the operand's own offset
                assert np.all(np.isnan(pre[ix["C"]])) if c["beta"] == 0.0 and "C" in c["fill"] else np.all(np.isfinite(pre[ix["C"]]))
                for o in c["poison"]:
                    assert np.all(np.isnan(pre[gr.indices(o, s.base, c["batch"])]))
                if c["A"]["sk"] == 2 and c["A"]["ld"] != 1:
                    assert np.all(np.isnan(pre[ix["A"] + 1])) or c["A"]["reg"] == c["B"]["reg"], case["name"]
                if kind == "exact":
                    v = pre[ix["A"]]
                    assert np.all(v == np.round(v)) and np.all(np.abs(v) >= 1) and np.all(np.abs(v) <= 7)
                A, B, C0, _ = s.operands(i, pre)
                if i + 1 < len(case["calls"]):       # stand in for the device: the contract's result, so that the next call starts from it
                    alpha, beta = gr.scalars(c, kind)
                    w = s.written(i)
                    out = gr.finish(A @ B, alpha, beta, np.where(w, C0, 0.0) if beta != 0.0 else None)
                    s.mem[ix["C"][w]] = out[w]
