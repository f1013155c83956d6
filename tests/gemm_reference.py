"""Operands and references of the pta_dgemm tests (tests/gemm_cases.py): test infrastructure, written from the contract in
include/pta_replicator_amd.h - C[b] = alpha A[b] op(B[b]) + beta C[b], A (m, k) at A[m lda + k ska], lower_only stores col <= row only -
not from any kernel.

NaN SLABS.  All buffers of a case live in ONE float64 allocation that is NaN wherever no operand element lies: between the rows of a
window (the columns left and right of it), in the other plane of an interleaved operand, and in guards of at least 128 rows of the
widest pitch in front of, between and behind the buffers - a read one column past K, one row past M or a whole tile too far stays
inside the allocation and meets NaN, which no finite result survives.  C holds its random values, or NaN everywhere when beta = 0.

EXACT.  Operand entries are non-zero integers in [-7, 7] and alpha, beta powers of two: every product and every partial sum is an
integer (a dyadic rational after alpha, beta) far below 2^53, so ANY order of summation, fused or not, gives the same double.  The
reference is the int64 product and the assertion is bit equality.  A dropped, doubled or misplaced k slot, an unmasked slot past K, a
wrong tile or a wrong beta changes an integer.

BOUND.  Entries +-U(0.5, 1.5), alpha = 0.7, beta = -1.3 (0 where the case has 0), the reference alpha sum_k a b + beta c in long double.
With u = 2^-53, per element
    |got - ref| <= (K + 3) u |alpha| sum_k |a||b| + 2 u |beta c|:
the accumulation rounds at most K times in any order, whether the matrix instruction fuses its four products or not (each rounding
is relative to a partial sum bounded by sum |a||b|), one more for a rounded product, one for alpha acc, one for the final fma, whose
rounding also falls on beta c; 2 u |beta c| covers an unfused beta c.  First order in u (K u < 1e-12 here).  Long double carries 11
more bits: the reference's own error is below 1/2048 of the bound.  Derived, not measured - it catches what integers cannot: an fp32
detour, an uncompensated conversion, a stale low word.

In both tests every element of the allocation that the call must not write - guards, the strict upper triangle under lower_only,
A and B, other batch members' surroundings - is compared with its pre-image through an int64 view (NaN payloads count), and everything
that must be written is finite."""
import numpy as np

import gemm_cases as gc

L = np.longdouble
U = 2.0 ** -53
BOUND_ALPHA, BOUND_BETA = 0.7, -1.3


def layout(case):
    """{region: first element}, total elements: the regions in order, each at an even element, guards of >= 128 rows of the widest
    pitch used inside the region (and of its neighbour) around each"""
    pitch = {r: 1 for r in case["regions"]}
    for c in case["calls"]:
        for o in (c["A"], c["B"], c["C"]) + c["poison"]:
            pitch[o["reg"]] = max(pitch[o["reg"]], o["ld"], o["sk"])
    base, at, prev = {}, 0, 0
    for r, size in case["regions"].items():
        at += gc.even(gc.GUARD_ROWS * max(prev, pitch[r]) + 16)
        base[r] = at
        at += gc.even(size)
        prev = pitch[r]
    return base, at + gc.even(gc.GUARD_ROWS * prev + 16)


def indices(o, base, batch):
    """flat element index of (b, i, j) of an operand, [batch, rows, cols]"""
    b, i, j = np.ogrid[:batch, :o["rows"], :o["cols"]]
    return base[o["reg"]] + o["off"] + b * o["stride"] + i * o["ld"] + j * o["sk"]


def scalars(call, kind):
    if kind == "exact":
        return call["alpha"], call["beta"]
    return BOUND_ALPHA, (BOUND_BETA if call["beta"] != 0.0 else 0.0)


def draw(rng, shape, kind):
    if kind == "exact":
        return (rng.integers(1, 8, shape) * rng.choice([-1, 1], shape)).astype(np.float64)
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def product_exact(A, B):
    """[batch, M, K] x [batch, K, N] of integer-valued doubles as the int64 product"""
    Ai, Bi = A.astype(np.int64), B.astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(Bi, B)
    return np.matmul(Ai, Bi)


def reference_exact(A, B, c, alpha, beta):
    p = alpha * product_exact(A, B).astype(np.float64)      # exact: integers below 2^53 times a power of two
    return p if beta == 0.0 else p + beta * c               # exact again: dyadic rationals of a few bits


def reference_bound(A, B, c, alpha, beta, K):
    """(reference in long double, the elementwise bound)"""
    ref = L(alpha) * np.matmul(A.astype(L), B.astype(L))
    mag = np.matmul(np.abs(A), np.abs(B)) * (1.0 + (K + 2) * U)       # fp64 sum of positive terms, pushed above the true sum
    bound = (K + 3) * U * abs(alpha) * mag
    if beta != 0.0:
        ref = ref + L(beta) * c.astype(L)
        bound = bound + 2 * U * np.abs(beta * c)
    return ref, bound


class Slab:
    """The allocation of one case under one kind of operands ("exact" or "bound"): prepare(i) poisons and fills for call i and returns the
    pre-image; check(i, pre, got) holds what the call left to the reference and returns the worst error over the bound (0 when exact)."""

    def __init__(self, case, kind, seed=0):
        self.case, self.kind = case, kind
        self.base, self.size = layout(case)
        self.rng = np.random.default_rng([seed, len(case["name"]), case["calls"][0]["K"], kind == "exact"])
        self.mem = np.full(self.size, np.nan)

    def idx(self, i):
        c = self.case["calls"][i]
        return {k: indices(c[k], self.base, c["batch"]) for k in "ABC"}

    def prepare(self, i):
        c = self.case["calls"][i]
        ix = self.idx(i)
        for o in c["poison"]:
            self.mem[indices(o, self.base, c["batch"])] = np.nan
        for k in c["fill"]:
            if k == "C" and c["beta"] == 0.0:
                self.mem[ix[k]] = np.nan
            else:
                self.mem[ix[k]] = draw(self.rng, ix[k].shape, self.kind)
        for k in "ABC":
            lo, hi = int(ix[k].min()), int(ix[k].max())
            assert lo >= gc.GUARD_ROWS and hi < self.size - gc.GUARD_ROWS, (self.case["name"], k)
        return self.mem.copy()

    def operands(self, i, pre):
        c = self.case["calls"][i]
        ix = self.idx(i)
        A, B, C0 = pre[ix["A"]], pre[ix["B"]], pre[ix["C"]]
        if c["transB"]:
            B = B.transpose(0, 2, 1)
        assert np.all(np.isfinite(A)) and np.all(np.isfinite(B)), self.case["name"]
        assert A.shape == (c["batch"], c["M"], c["K"]) and B.shape == (c["batch"], c["K"], c["N"])
        return A, B, C0, ix["C"]

    def written(self, i):
        c = self.case["calls"][i]
        return np.broadcast_to(np.tril(np.ones((c["M"], c["N"]), bool)) if c["lower"] else np.ones((c["M"], c["N"]), bool),
                               (c["batch"], c["M"], c["N"]))

    def check(self, i, pre, got):
        """`got`: the allocation after call i.  Adopts it as the state the next call starts from."""
        c = self.case["calls"][i]
        name = (self.case["name"], i, self.kind)
        alpha, beta = scalars(c, self.kind)
        A, B, C0, ixc = self.operands(i, pre)
        w = self.written(i)
        out = got[ixc]
        assert np.all(np.isfinite(out[w])), (name, "not finite", int(np.sum(~np.isfinite(out[w]))))
        untouched = np.ones(self.size, bool)
        untouched[ixc[w]] = False
        same = bits(got)[untouched] == bits(pre)[untouched]
        assert np.all(same), (name, "written outside", np.flatnonzero(untouched)[~same][:8])
        if beta != 0.0:
            assert np.all(np.isfinite(C0[w])), name
        cw = np.where(w, C0, 0.0) if beta != 0.0 else None
        worst = 0.0
        if self.kind == "exact":
            ref = reference_exact(A, B, cw, alpha, beta)
            bad = bits(out)[w] != bits(ref)[w]
            assert not np.any(bad), (name, "differs from the integer product", int(bad.sum()), np.argwhere(bad.reshape(-1))[:4].ravel(),
                                     out[w][bad][:4], ref[w][bad][:4])
        else:
            ref, bound = reference_bound(A, B, cw, alpha, beta, c["K"])
            ratio = (np.abs(out.astype(L) - ref) / bound).astype(np.float64)[w]
            worst = float(ratio.max())
            assert worst <= 1.0, (name, "outside the bound", worst)
        self.mem = got.copy()
        return worst


# ---------------------------------------------------------------- honest fp64 products and seeded defects (the host test) --------
def finish(acc, alpha, beta, c):
    v = alpha * acc
    return v if beta == 0.0 else v + beta * c


def product_orders(A, B):
    """sum_k a b of [M, K] x [K, N] in fp64, four honest ways"""
    M, K = A.shape
    out = {"numpy": A @ B}
    acc = np.zeros((M, B.shape[1]))
    for k in range(K):          # a sequential chain with one rounding per term (the product held in long double: fma-like)
        acc = (A[:, k, None].astype(L) * B[k].astype(L) + acc.astype(L)).astype(np.float64)
    out["chain"] = acc
    terms = [A[:, k, None] * B[k] for k in range(K)]
    while len(terms) > 1:       # pairwise
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    out["pairwise"] = terms[0]
    acc = np.zeros((M, B.shape[1]))
    for k0 in range(0, K, 4):   # four products summed before one rounding into the accumulator: the matrix instruction's blocks
        s = acc.astype(L)
        for k in range(k0, min(k0 + 4, K)):
            s = s + A[:, k, None].astype(L) * B[k].astype(L)
        acc = s.astype(np.float64)
    out["blocks of 4"] = acc
    return out


def seeded_defects(Aw, Bw, c, alpha, beta, K):
    """{defect: result}: Aw [M, K + 1], Bw [K + 1, N] are the operands with the neighbouring column / row behind K (finite here)"""
    A, B = Aw[:, :K], Bw[:K]
    sw = A.copy()
    sw[:, [1, K - 2]] = sw[:, [K - 2, 1]]
    f32 = A.copy()
    f32[0, K // 2] = np.float32(f32[0, K // 2])
    return {
        "last k term dropped": finish(A[:, :K - 1] @ B[:K - 1], alpha, beta, c),
        "slot K read from the neighbouring column": finish(Aw @ Bw, alpha, beta, c),
        "two k slots swapped in A only": finish(sw @ B, alpha, beta, c),
        "beta applied as 0": finish(A @ B, alpha, 0.0, c),
        "one element rounded to fp32": finish(f32 @ B, alpha, beta, c),
    }
