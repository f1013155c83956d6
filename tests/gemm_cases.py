"""The shapes and operand layouts at which pta_dgemm reaches each of its nine kernel instances, each lower mode, both sides of each
threshold and every caller's form.

pta_dgemm_launch picks the instance from algo, from M >= 256, N >= 128, K >= 32 and from the `vec` predicate (transB, ska == 1, even K,
lda, ldb, strideA, strideB, A and B 16-byte aligned).  tests/test_gemm_cases.py asks pta_dgemm_plan (no device call) that every case
below reaches the instance it names and that together they cover the lot; tests/test_gpu_gemm_reference.py runs every case on the
NaN slabs of tests/gemm_reference.py.

A case is {"name", "regions", "calls", "deep"}.  `regions` names the buffers, {name: elements}; gemm_reference.layout puts them, each
between guards, into ONE allocation at even element offsets, so an operand is 16-byte aligned exactly when its own offset is even.
`calls` are the pta_dgemm calls in the caller's order on that one allocation (one call, except for the idft and clnl forms).  A call is
    transB, M, N, K, algo, lower, batch, alpha, beta        alpha, beta: the exact test's (powers of two; beta = 0 stays 0 in the bound test)
    A, B, C        operands: {"reg", "off", "ld", "sk", "stride", "rows", "cols"}: element (b, i, j) at reg + off + b stride + i ld + j sk
    fill           the operands given fresh values before this call (the others keep what the allocation holds: an earlier call's output)
    poison         windows set to NaN before this call (the plane of an interleaved operand that this call must not read)
    expect         the plan values the call exists for (a subset of the plan's keys; kernel and lower by name)
`deep` cases (K in the thousands) run the exact test only: the bound grows like K^2 and stops telling an honest product from a wrong one."""
# plan["kernel"] and plan["lower_mode"] of pta_dgemm_plan by name (pta_replicator_amd._lib holds the same tuples)
DGEMM_KERNELS = ("k_dgemm_valu<false>", "k_dgemm_valu<true>", "k_dgemm_mfma<false>", "k_dgemm_mfma<true>", "k_dgemm_mfma128<false,false>",
                 "k_dgemm_mfma128<true,false>", "k_dgemm_mfma128<true,true>", "k_dgemm_glds128<false,0>", "k_dgemm_glds128<false,1>")
DGEMM_LOWER = ("none", "grid2d", "triangle", "trapezoid")

VALU_N, VALU_T, MFMA_N, MFMA_T, M128_N, M128_T, M128_TV, GLDS_E0, GLDS_E1 = DGEMM_KERNELS
L_NONE, L_GRID2D, L_TRIANGLE, L_TRAPEZOID = DGEMM_LOWER
TILE128 = (M128_N, M128_T, M128_TV, GLDS_E0, GLDS_E1)
ALPHAS = (1.0, -1.0, 0.5, 2.0)
BETAS = (0.0, 1.0, -1.0, 0.5, 2.0)
GUARD_ROWS = 128


def cdiv(a, b):
    return -(-a // b)


def even(v):
    return v + (v & 1)


def op(reg, off, ld, rows, cols, sk=1, stride=0):
    return dict(reg=reg, off=int(off), ld=int(ld), sk=int(sk), stride=int(stride), rows=int(rows), cols=int(cols))


def span(o, batch):
    """elements from the operand's origin to the end of its last element"""
    return (batch - 1) * o["stride"] + (o["rows"] - 1) * o["ld"] + (o["cols"] - 1) * o["sk"] + 1


def call(transB, M, N, K, algo, A, B, C, lower=0, batch=1, alpha=1.0, beta=1.0, fill=("A", "B", "C"), poison=(), **expect):
    return dict(transB=transB, M=M, N=N, K=K, algo=algo, lower=lower, batch=batch, alpha=alpha, beta=beta, A=A, B=B, C=C, fill=tuple(fill),
                poison=tuple(poison), expect=expect)


def plan_args(c):
    """the arguments of pta_dgemm_plan for a call (regions start at even elements: the operand's own offset decides its alignment)"""
    return (c["transB"], c["M"], c["N"], c["K"], c["A"]["ld"], c["A"]["sk"], c["B"]["ld"], c["A"]["stride"], c["B"]["stride"],
            8 * (c["A"]["off"] & 1), 8 * (c["B"]["off"] & 1), c["lower"], c["algo"], c["batch"])


def plan(c):
    from pta_replicator_amd import _lib
    p = _lib.launch_plan("pta_dgemm", *plan_args(c))
    p["kernel"], p["lower_mode"] = DGEMM_KERNELS[p["kernel"]], DGEMM_LOWER[p["lower_mode"]]
    return p


CASES = []


def add(name, regions, calls, deep=False):
    i = len(CASES)
    for j, c in enumerate(calls):   # the exact test's scalars walk their sets unless the caller's form fixes them
        if c["alpha"] is None:
            c["alpha"] = ALPHAS[(i + j) % 4]
        if c["beta"] is None:
            c["beta"] = BETAS[(i + j) % 5]
    CASES.append(dict(name=name, regions=regions, calls=list(calls), deep=deep))


def plain(name, transB, M, N, K, algo, lower=0, batch=1, alpha=None, beta=None, a_off=4, b_off=2, lda=None, ldb=None, ska=1, sA=None, sB=None,
          **expect):
    """A, B and C each a window of an own wider buffer: A at column a_off of rows lda = K ska + 22 wide, B at column b_off of rows K + 6
    (transB) or N + 6 wide, C at column 3 of rows N + 5 wide; batch members one after the other."""
    lda = K * ska + 22 if lda is None else lda
    ldb = (K + 6 if transB else N + 6) if ldb is None else ldb
    ldc = N + 5
    brows = N if transB else K
    sA = even(M * lda) if sA is None else sA
    sB = even(brows * ldb) if sB is None else sB
    sC = M * ldc + 7
    A = op("A", a_off, lda, M, K, ska, sA)
    B = op("B", b_off, ldb, N, K, 1, sB) if transB else op("B", b_off, ldb, K, N, 1, sB)
    C = op("C", 3, ldc, M, N, 1, sC)
    regions = {"A": a_off + span(A, batch) + 8, "B": b_off + span(B, batch) + 8, "C": 3 + span(C, batch) + 8}
    add(name, regions, [call(transB, M, N, K, algo, A, B, C, lower, batch, alpha, beta, **expect)])


# ---------------------------------------------------------------- the two VALU kernels and the two 64-tile kernels -------------
for _tb, _valu, _mfma in ((0, VALU_N, MFMA_N), (1, VALU_T, MFMA_T)):
    plain(f"valu tb{_tb} 5x7x3", _tb, 5, 7, 3, 0, kernel=_valu, tile=0, lower_mode=L_NONE)
    plain(f"valu tb{_tb} 70x130x37 batch 2", _tb, 70, 130, 37, 0, batch=2, kernel=_valu, grid_x=2)
    plain(f"valu tb{_tb} lower 65x65x17", _tb, 65, 65, 17, 0, lower=1, kernel=_valu, lower_mode=L_GRID2D)
    plain(f"valu tb{_tb} ska 2", _tb, 33, 20, 9, 0, ska=2, a_off=3, kernel=_valu)
    # M and N one below, at and one above the 64 tile; K below one slab, one slab, a tail, two slabs, two and a tail
    for _M, _N, _K in ((63, 65, 15), (64, 64, 16), (65, 63, 17), (1, 1, 1), (129, 127, 32), (64, 129, 37)):
        plain(f"mfma tb{_tb} {_M}x{_N}x{_K}", _tb, _M, _N, _K, 1, kernel=_mfma, tile=64, lower_mode=L_NONE, grid_x=cdiv(_N, 64))
    plain(f"mfma tb{_tb} lower 130x130x21 batch 2", _tb, 130, 130, 21, 1, lower=1, batch=2, kernel=_mfma, lower_mode=L_GRID2D, grid_x=3)
    plain(f"mfma tb{_tb} lower 65x130x16 (M < N)", _tb, 65, 130, 16, 2, lower=1, kernel=_mfma, lower_mode=L_GRID2D)
    plain(f"mfma tb{_tb} ska 2 odd offset", _tb, 70, 33, 19, 1, ska=2, a_off=3, kernel=_mfma)
    # algo 2 and 3 below the thresholds are the 64-tile kernel too
    plain(f"mfma tb{_tb} algo 3 200x130x34", _tb, 200, 130, 34, 3, kernel=_mfma, tile=64)


# ---------------------------------------------------------------- each threshold from both sides, algo 1 and 2 ------------------
# transB = 1 with every vec condition met: at or above all three thresholds algo 1 is the 16-byte-load kernel and algo 2 the DMA kernel
THRESHOLDS = {(256, 128, 32): True, (255, 128, 32): False, (256, 127, 32): False, (256, 128, 31): False, (255, 127, 31): False}
for (_M, _N, _K), _big in THRESHOLDS.items():
    for _algo in (1, 2):
        _k = (M128_TV if _algo == 1 else GLDS_E0) if _big else MFMA_T
        plain(f"threshold {_M}x{_N}x{_K} algo {_algo}", 1, _M, _N, _K, _algo, kernel=_k, tile=128 if _big else 64)
    _k = M128_N if _big else MFMA_N
    plain(f"threshold tb0 {_M}x{_N}x{_K}", 0, _M, _N, _K, 1, kernel=_k, tile=128 if _big else 64)


# ---------------------------------------------------------------- each vec condition failing alone -----------------------------
VEC_SHAPE = (257, 129, 34)          # two row tiles (the last of one row), two column tiles (the last of one column), 2 slabs and a tail
VEC_FAIL = {
    "ska 2": dict(ska=2),
    "odd K": dict(K=35, lda=34 + 22, ldb=34 + 6),
    "odd lda": dict(lda=34 + 23),
    "odd ldb": dict(ldb=34 + 7),
    "odd strideA": dict(sA=257 * (34 + 22) + 1, batch=2),
    "odd strideB": dict(sB=129 * (34 + 6) + 1, batch=2),
    "A 8 bytes off": dict(a_off=5),
    "B 8 bytes off": dict(b_off=3),
}
for _algo in (1, 2, 3):
    _M, _N, _K = VEC_SHAPE
    plain(f"vec all met algo {_algo}", 1, _M, _N, _K, _algo, batch=2, kernel=(M128_TV, GLDS_E0, GLDS_E1)[_algo - 1], tile=128, lower_mode=L_NONE, grid_x=2)
    for _why, _kw in VEC_FAIL.items():
        if _algo == 3 and _why not in ("odd K", "A 8 bytes off"):
            continue
        _kw = dict(_kw)
        plain(f"vec fails: {_why}, algo {_algo}", 1, _M, _N, _kw.pop("K", _K), _algo, kernel=M128_T, tile=128, **_kw)


# ---------------------------------------------------------------- slab counts 2, 3, 4 of the 128-tile kernels, with and without a tail
SLAB_K_EVEN = (32, 48, 64, 46, 62, 34)      # nslab 2, 3, 4 without a tail; 3, 4, 3 with one (both parities of the last buffer)
SLAB_K_QUAD = (36, 40, 44)                  # tails of 4, 8, 12: K ends where one k-quad of the matrix instruction's lanes hands over to the next
SLAB_K_ODD = (33, 47)                       # the scalar kernels only: 3 slabs, tails of 1 and 15


def _slab(kernel, K):
    M, N = 257, 129
    if kernel == M128_N:
        plain(f"slabs {kernel} K={K}", 0, M, N, K, 1, kernel=kernel, tile=128, grid_x=2)
    elif kernel == M128_T:   # transB without vec: A one element off
        plain(f"slabs {kernel} K={K}", 1, M, N, K, 1 + K % 2, a_off=5, kernel=kernel, tile=128, grid_x=2)
    else:
        plain(f"slabs {kernel} K={K}", 1, M, N, K, {M128_TV: 1, GLDS_E0: 2, GLDS_E1: 3}[kernel], kernel=kernel, tile=128, grid_x=2)


for _kern in TILE128:
    for _K in SLAB_K_EVEN + SLAB_K_QUAD + (SLAB_K_ODD if _kern in (M128_N, M128_T) else ()):
        _slab(_kern, _K)


# ---------------------------------------------------------------- M and N around the 128 tile, the lower modes ------------------
EDGE_MN = ((256, 128), (300, 257), (383, 300), (385, 128))      # at a multiple; above both; one below / well above; one above / at
for _kern, _tb, _algo, _kw in ((M128_N, 0, 1, {}), (M128_T, 1, 2, dict(b_off=3)), (M128_TV, 1, 1, {}), (GLDS_E0, 1, 2, {}), (GLDS_E1, 1, 3, {})):
    for _M, _N in EDGE_MN:
        plain(f"edges {_kern} {_M}x{_N}x36", _tb, _M, _N, 36, _algo, kernel=_kern, tile=128, lower_mode=L_NONE, grid_x=cdiv(_N, 128), grid_y=cdiv(_M, 128),
              **_kw)
    # lower_only on a square C: the 1-D triangle (3 tile rows = 6 workgroups; 300 = two tiles and 44 rows)
    plain(f"triangle {_kern} 300x300x40", _tb, 300, 300, 40, _algo, lower=1, batch=2, kernel=_kern, lower_mode=L_TRIANGLE, grid_x=6, grid_y=1, **_kw)
    # lower_only with M < N: the 2-D grid, tiles above the diagonal leave at once
    plain(f"2-D early exit {_kern} 256x300x32", _tb, 256, 300, 32, _algo, lower=1, kernel=_kern, lower_mode=L_GRID2D, grid_x=3, grid_y=2, **_kw)
# lower_only with M > N is the 2-D grid on the three register-staging kernels
plain("2-D early exit M > N, mfma128 vec", 1, 300, 130, 46, 1, lower=1, kernel=M128_TV, lower_mode=L_GRID2D, grid_x=2, grid_y=3)
plain("2-D early exit M > N, mfma128 scalar", 1, 300, 130, 46, 2, lower=1, a_off=5, kernel=M128_T, lower_mode=L_GRID2D, grid_x=2, grid_y=3)
plain("2-D early exit M > N, transB 0", 0, 300, 130, 46, 2, lower=1, kernel=M128_N, lower_mode=L_GRID2D, grid_x=2, grid_y=3)


# ---------------------------------------------------------------- the callers' forms -------------------------------------------
def gram(name, M, K, deep=False, **expect):
    """engine_td.py: S = T^T T on the lower triangle, T [K, ldt]: A (m, k) = T[k ldt + m] (lda = 1, ska = ldt), B = the same pointer"""
    ldt = M + 9
    A = op("T", 2, 1, M, K, ldt)
    B = op("T", 2, ldt, K, M)
    C = op("S", 1, M + 3, M, M)
    add(name, {"T": 2 + K * ldt, "S": 1 + M * (M + 3)}, [call(0, M, M, K, 1, A, B, C, lower=1, alpha=1.0, beta=0.0, **expect)], deep=deep)


gram("TtT 37x37x40", 37, 40, kernel=MFMA_N, lower_mode=L_GRID2D)
gram("TtT 257x257x34", 257, 34, kernel=M128_N, lower_mode=L_TRIANGLE, grid_x=6)
gram("TtT 130x130x6002 (the production depth)", 130, 6002, deep=True, kernel=MFMA_N, lower_mode=L_GRID2D)


def idft(name, M, N, Kf, algo, **expect):
    """pta_gwb_kernels.hip: g = Re-plane(W) T[:Kf] then g += Im-plane(W) T[Kf:], W rows of interleaved pairs read from elements 2 and 3"""
    ldw, ldt, ldg = 2 * Kf + 6, N + 4, N + 2
    Are, Aim = op("W", 2, ldw, M, Kf, 2), op("W", 3, ldw, M, Kf, 2)
    B0, B1 = op("T", 0, ldt, Kf, N), op("T", Kf * ldt, ldt, Kf, N)
    C = op("G", 0, ldg, M, N)
    add(name, {"W": M * ldw, "T": 2 * Kf * ldt, "G": M * ldg},
        [call(0, M, N, Kf, algo, Are, B0, C, alpha=1.0, beta=0.0, fill=("A", "B", "C"), poison=(Aim,), **expect),
         call(0, M, N, Kf, algo, Aim, B1, C, alpha=1.0, beta=1.0, fill=("A", "B"), poison=(Are,), **expect)])


idft("idft 68x70x29", 68, 70, 29, 1, kernel=MFMA_N)
idft("idft 68x70x29 valu", 68, 70, 29, 0, kernel=VALU_N)
idft("idft 257x130x33", 257, 130, 33, 1, kernel=M128_N)


def mix(name, P, npts, algo, shared, **expect):
    """pta_gwb_kernels.hip / pta_gwb_aniso_kernels.hip: G[r] = M G0[r] (shared factor, sA = 0) or M[r] G0[r] (sA = ld_m), batch 3"""
    ldg, ld_m = npts + 3, P * P + 5
    sr = P * ldg + 1
    A = op("M", 0, P, P, P, 1, 0 if shared else ld_m)
    B = op("G0", 1, ldg, P, npts, 1, sr)
    C = op("G", 1, ldg, P, npts, 1, sr)
    add(name, {"M": 3 * ld_m, "G0": 1 + 3 * sr, "G": 1 + 3 * sr}, [call(0, P, npts, P, algo, A, B, C, batch=3, alpha=1.0, beta=0.0, **expect)])


for _P in (3, 17, 68):
    for _algo, _k in ((0, VALU_N), (1, MFMA_N)):
        mix(f"mix P={_P} algo {_algo} shared factor", _P, 70, _algo, True, kernel=_k)
        mix(f"mix P={_P} algo {_algo} factor per realisation", _P, 70, _algo, False, kernel=_k)


def clnl(name, j0, R, blocks, **expect):
    """pta_clnl_kernels.hip: V[j0 : j0 + M] -= L[j0 : j0 + M, :j0] V[:j0] per grid point, B and C windows of ONE buffer, block after block:
    the second call's B holds the rows the first wrote"""
    n = j0 + sum(blocks)
    ld_v = R + 3
    calls, j = [], j0
    for i, M in enumerate(blocks):
        A = op("L", j * n, n, M, j, 1, n * n)
        B = op("V", 0, ld_v, j, R, 1, n * ld_v)
        C = op("V", j * ld_v, ld_v, M, R, 1, n * ld_v)
        calls.append(call(0, M, R, j, 1, A, B, C, batch=3, alpha=-1.0, beta=1.0, fill=("A", "B", "C") if i == 0 else ("A", "C"), **expect))
        j += M
    add(name, {"L": 3 * n * n, "V": 3 * n * ld_v}, calls)


clnl("clnl j0=64, blocks of 64 and 5", 64, 33, (64, 5), kernel=MFMA_N, lower_mode=L_NONE)


def syrk(name, M, N, K, algo, **expect):
    """pta_potrf.hip: A22 -= L21 L21^T on the lower triangle, L21 a column block of the matrix and A22 the block right of it, batch 2"""
    c0 = 6
    n, ld = 40 + M, even(c0 + K + N + 10)
    A = op("X", 40 * ld + c0, ld, M, K, 1, n * ld)
    B = op("X", 40 * ld + c0, ld, N, K, 1, n * ld)
    C = op("X", 40 * ld + c0 + K, ld, M, N, 1, n * ld)
    add(name, {"X": 2 * n * ld}, [call(1, M, N, K, algo, A, B, C, lower=1, batch=2, alpha=-1.0, beta=1.0, **expect)])


for _algo, _k in ((1, M128_TV), (2, GLDS_E0), (3, GLDS_E1)):
    syrk(f"syrk 300x300x46 algo {_algo}", 300, 300, 46, _algo, kernel=_k, lower_mode=L_TRIANGLE, grid_x=6)
    syrk(f"syrk 300x130x46 algo {_algo}", 300, 130, 46, _algo, kernel=_k, lower_mode=L_GRID2D if _algo == 1 else L_TRAPEZOID, grid_x=2 if _algo == 1 else 5)
    syrk(f"syrk 515x257x64 algo {_algo}", 515, 257, 64, _algo, kernel=_k, lower_mode=L_GRID2D if _algo == 1 else L_TRAPEZOID, grid_x=3 if _algo == 1 else 12)


def trmm(name, R, N, algo, beta, **expect):
    """pta_td_trmm: out = z L^T (+ out), R realisations of a factor of order N"""
    A = op("z", 2, N + 4, R, N)
    B = op("L", 0, N, N, N)
    C = op("out", 1, N + 3, R, N)
    add(name, {"z": 2 + R * (N + 4), "L": N * N, "out": 1 + R * (N + 3)}, [call(1, R, N, N, algo, A, B, C, alpha=1.0, beta=beta, **expect)])


trmm("trmm 17x130x130", 17, 130, 1, 0.0, kernel=MFMA_T)
trmm("trmm 17x130x130 accumulate", 17, 130, 1, 1.0, kernel=MFMA_T)
trmm("trmm 17x130x130 valu", 17, 130, 0, 0.0, kernel=VALU_T)
