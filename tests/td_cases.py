"""Hand-built inputs of the TD reference tests (tests/td_reference.py): matrix families, the fp64 emulations of the algorithm
classes the bounds are derived for, and the case tables the GPU file walks.  NumPy only.

Families, each a function of (n, seed) returning a dict with the fp64 matrix A and what it was assembled from:
  W   the suite's Wishart, X X^T + 0.1 I with X [n, n + 5]                                             cond(700) ~ 1e4
  Q   quiet TD covariance F diag(phi) F^T + sigma^2 I + ECORR: 30 sine and 30 cosine columns at k / T over T = 15 yr of unevenly
      spaced TOAs, power law gamma = 4.33, log10_A = -14, sigma = 1e-7 s, ECORR 1e-7 s on epochs of 4 TOAs   cond(700) ~ 2.5e5
  Lo  loud: log10_A = -12.5, sigma = 3e-8 s, no ECORR                                                    cond(700) ~ 2.7e9
  X   Lo with sigma = 1e-9 s: LAPACK's dpotrf factors it at every order used (test_td_reference_host checks) cond(700) ~ 1e12
      - for the conventional (bound (s)) schedules only
The TD families are in seconds^2 (entries 1e-14 .. 1e-9): nothing in a residual test depends on the scale."""
import numpy as np

YR = 365.25 * 86400.0
FYR = 1.0 / YR
FAMILIES = ("W", "Q", "Lo", "X")
_TD = {"Q": dict(log10_A=-14.0, sigma=1e-7, ecorr=1e-7), "Lo": dict(log10_A=-12.5, sigma=3e-8, ecorr=None),
       "X": dict(log10_A=-12.5, sigma=1e-9, ecorr=None)}


def powerlaw_phi(T, ncomp, log10_A, gamma):
    """prior variance of the sine and cosine coefficient at f_k = k / T, k = 1 .. ncomp (s^2): A^2 / (12 pi^2) f_yr^(gamma-3) f^-gamma / T"""
    f = np.arange(1, ncomp + 1) / T
    return f, (10.0 ** log10_A) ** 2 / (12 * np.pi ** 2) * FYR ** (gamma - 3) * f ** (-gamma) / T


def td_inputs(n, seed, log10_A, sigma, ecorr, ncomp=30, gamma=4.33, epoch=4, shuffle=False):
    """Ft [2 ncomp, n], phi [2 ncomp], sigma2 [n], epoch_of / ecorr2 [n] (None without ECORR) of one pulsar"""
    rng = np.random.default_rng(seed)
    T = 15 * YR
    t = np.sort(rng.uniform(0.0, T, n))
    epoch_of = np.arange(n) // epoch
    if shuffle:
        perm = rng.permutation(n)
        t, epoch_of = t[perm], epoch_of[perm]
    f, p = powerlaw_phi(T, ncomp, log10_A, gamma)
    arg = 2 * np.pi * f[:, None] * t[None, :]
    Ft = np.empty((2 * ncomp, n))
    Ft[0::2], Ft[1::2] = np.sin(arg), np.cos(arg)
    d = dict(Ft=Ft, phi=np.repeat(p, 2), sigma2=np.full(n, sigma ** 2), epoch_of=None, ecorr2=None)
    if ecorr is not None:
        d["epoch_of"], d["ecorr2"] = epoch_of.astype(np.int32), np.full(n, ecorr ** 2)
    return d


def cov_fp64(d):
    C = (d["Ft"].T * d["phi"]) @ d["Ft"] + np.diag(d["sigma2"])
    if d["epoch_of"] is not None:
        C = C + np.where(d["epoch_of"][:, None] == d["epoch_of"][None, :], d["ecorr2"][:, None], 0.0)
    return 0.5 * (C + C.T)


def family(name, n, seed=0, **kw):
    """dict(A=fp64 SPD matrix [n, n], ...) of family `name`"""
    if name == "W":
        Xm = np.random.default_rng(1000 * seed + n).standard_normal((n, n + 5))
        return dict(A=Xm @ Xm.T + 0.1 * np.eye(n))
    d = td_inputs(n, 1000 * seed + n, **{**_TD[name], **kw})
    d["A"] = cov_fp64(d)
    return d


# ---- fp64 emulations of the algorithm classes (NumPy, one rounding per operation as far as BLAS allows) ----
def chol_unblocked(A):
    """conventional Cholesky, column by column (class (s))"""
    A = np.tril(A).copy()
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(j + 1)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _inv_lower(T):
    """fp64 inverse of a lower triangle, every column by forward substitution (Method 1)"""
    w = T.shape[0]
    X = np.zeros_like(T)
    for i in range(w):
        r = -(T[i, :i] @ X[:i])
        r[i] += 1.0
        X[i] = r / T[i, i]
    return X


def _inv_block(L11):
    """the block form W = [[X1, 0], [-X2 (L21 X1), X2]] of a group wider than 64 columns"""
    w = L11.shape[0]
    if w <= 64:
        return _inv_lower(L11)
    m = w - 64
    X1, X2 = _inv_lower(L11[:m, :m]), _inv_lower(L11[m:, m:])
    W = np.zeros_like(L11)
    W[:m, :m], W[m:, m:] = X1, X2
    W[m:, :m] = -(X2 @ (L11[m:, :m] @ X1))
    return W


def _diag_block(Ag):
    """a group's diagonal block: base blocks conventionally, the second one's rows by a product with the first's inverse"""
    w = Ag.shape[0]
    if w <= 64:
        return chol_unblocked(Ag)
    m = w - 64
    L = np.zeros_like(Ag)
    L[:m, :m] = chol_unblocked(Ag[:m, :m])
    L[m:, :m] = Ag[m:, :m] @ _inv_lower(L[:m, :m]).T
    L[m:, m:] = chol_unblocked(Ag[m:, m:] - L[m:, :m] @ L[m:, :m].T)
    return L


def chol_block_inverse(A, b, left=False):
    """blocked Cholesky over the end-aligned b-column groups whose rows below a diagonal block are a product with its explicit
    inverse (class (w)); right-looking, or left-looking (a block column updated once with everything to its left)"""
    from td_reference import groups
    A = np.tril(A) + np.tril(A, -1).T
    n = A.shape[0]
    L = np.zeros_like(A)
    for c0, c1 in groups(n, b):
        blk = A[c0:, c0:c1].copy()
        if left:
            blk -= L[c0:, :c0] @ L[c0:c1, :c0].T
        L[c0:c1, c0:c1] = _diag_block(np.tril(blk[:c1 - c0]))
        if c1 < n:
            L[c1:, c0:c1] = blk[c1 - c0:] @ _inv_block(L[c0:c1, c0:c1]).T
            if not left:
                A[c1:, c1:] -= L[c1:, c0:c1] @ L[c1:, c0:c1].T
    return L


EMULATIONS = {"unblocked": (chol_unblocked, None), "inverse64": (lambda A: chol_block_inverse(A, 64), 64),
              "inverse128": (lambda A: chol_block_inverse(A, 128), 128), "left128": (lambda A: chol_block_inverse(A, 128, left=True), 128)}

# ---- case tables ----
WS_ORDERS = (258, 300, 384, 386, 520, 700, 385)         # 256-column panels: the workspace scheme from n = 258; 385: scalar operands
WS_SCHEDULES = ("LEFT", "LEFT|LEFT_SPLIT", "LEFT|DIAG_AHEAD", "LEFT|SOLVE_ROWS", "DIAG_AHEAD", "DIAG_AHEAD|SOLVE_ROWS", "DIAG64", "EPI1",
                "REG_STAGING", "CHAINS1", "CHAINS3", "CHAINS4")
WS_BATCHES = (1, 3, 5)
WIDE_CASES = ((1026, "LEFT"), (1026, "0"), (1290, "LEFT"), (1290, "0"))     # default 1024-column panels
EX_ORDERS = (1, 2, 63, 64, 65, 128, 130, 200, 515)
EX_FLAGS = ("0", "SUBSTITUTION", "VALU", "NO_LOOKAHEAD")
RAGGED_ORDERS = ((258, 130, 64, 2, 520, 384), (700, 698, 256, 254))
RAGGED_FLAGS = ("0", "LEFT", "CHAINS3", "NO_LOOKAHEAD")
FUSED_ORDERS, FUSED_KF = (386, 520), (0, 29, 60, 64)
ASM_K, ASM_ORDERS = (1, 2, 29, 40, 60, 64), (2, 254, 256, 258, 514)     # K = 40: the walk kernel's 12 k-steps (K = 33 .. 48)
DRAW_ORDERS, DRAW_R = (1, 2, 17, 256, 257, 513), (1, 5, 70)
ORF_ORDERS = (1, 2, 17, 80, 81, 130)                    # pta_gwb_orf_factor: the LDS factorisation up to P = 80, the batched one above


def flag_bits(lib, names):
    """"LEFT|SOLVE_ROWS", "CHAINS3", "0" ... -> the PTA_POTRF_* bits"""
    fl = 0
    for nm in names.split("|"):
        if nm == "0":
            continue
        fl |= lib.POTRF_CHAINS(int(nm[6:])) if nm.startswith("CHAINS") else getattr(lib, "POTRF_" + nm)
    return fl
