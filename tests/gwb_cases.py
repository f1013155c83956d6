"""Hand-built calls of the GWB frequency-to-time stage: the operands tests/test_gwb_reference_host.py (CPU) and
tests/test_gpu_gwb_direct.py (MI355X) evaluate against tests/gwb_reference.py - test infrastructure, not product code.

A case is (Nf, npts, i0, R, P, r0, ldg - npts, extras): sqrtC of order 1e-7 from a seeded generator, nonzero in every bin (DC and
Nyquist too: the contract never reads them, so a kernel that does is seen), draws O(1), dt = 977 s.  extras: scale = ld_scale - Nf
of a per-realisation spectrum with visibly different rows and NaN in column 0 and in every column from Nf - 1 on; fast = rng_fast;
rows = the rows the reference is evaluated for when R P is large (the call still computes them all).  The large shapes keep R P <= 12
so that a reference costs a second; the rows beyond one wave (P >= 65) ride on a shape small enough for 130 of them.

  A  fit edges: Kf + npts - 2 = 4095 (3499, 600) - 4096 is refused; Nf = 3, 4 with npts = 1, 2
  B  Kf = 511, 512, 513, 1024, 1025 around the 512-strided first butterfly (the one 512-block that straddles Kf)
  C  i0 = 1, 2, 10, 3400, i0 > Kf; i0 = 0 for the DFT-GEMM kernels alone (chirp-z refuses it)
  D  the window against 1024 (the pruned last butterfly): i0 - 2 + npts = 1023, 1024, 1025 at i0 = 10 and at i0 = 1, npts = 1015 and
     1016 at i0 = 1, a window wholly above 1024, 37 samples of which only output 0 is ever stored
  E  P = 1, 3, 65, 66; R P = 7, 9, 65, 132 (no multiple of the 16 rows of a wave or the 64 of a workgroup); r0 = 2^32 + 5
  F  ldg = npts + 5 into a NaN-filled buffer
  G  scale: R = 3 and 4 rows, ld_scale = Nf - 1 and Nf + 3
  H  rng_fast = 1"""
import numpy as np

from gwb_reference import FFT_N

DT = 977.0
INV_DT = 1.0 / DT
SEED = 0x9E3779B97F4A7C15
BIG = 2 ** 32 + 5


def _c(name, Nf, npts, i0, R=2, P=3, r0=12345, pad=0, **extras):
    return dict(name=name, Nf=Nf, npts=npts, i0=i0, R=R, P=P, r0=r0, pad=pad, extras=extras)


CASES = [
    # A
    _c("A-fit4095", 3499, 600, 10, R=1, P=3, pad=5),
    _c("A-nf3-n1", 3, 1, 1, pad=5), _c("A-nf3-n2", 3, 2, 2), _c("A-nf4-n1", 4, 1, 10), _c("A-nf4-n2", 4, 2, 1, r0=BIG),
    # B
    _c("B-kf511", 513, 40, 10), _c("B-kf512", 514, 41, 10, pad=5), _c("B-kf513", 515, 33, 10), _c("B-kf1024", 1026, 1015, 10),
    _c("B-kf1025", 1027, 70, 10),
    # C
    _c("C-i0-1", 500, 37, 1), _c("C-i0-2", 601, 200, 2, pad=5), _c("C-i0-10", 3000, 600, 10, r0=BIG), _c("C-i0-3400", 600, 600, 3400),
    _c("C-i0-above-kf", 40, 50, 100), _c("C-i0-0", 601, 200, 0, pad=5),
    # D
    _c("D-1024", 700, 1016, 10), _c("D-1025", 700, 1017, 10, pad=5), _c("D-i1-1015", 300, 1015, 1), _c("D-i1-1016", 300, 1016, 1),
    _c("D-i1-1023", 300, 1024, 1), _c("D-i1-1024", 300, 1025, 1, pad=5), _c("D-i1-1025", 300, 1026, 1), _c("D-above", 300, 100, 1100),
    _c("D-37", 500, 37, 10), _c("D-crosses", 2000, 1100, 10, R=1),
    # E
    _c("E-p1", 601, 200, 10, R=7, P=1, r0=BIG, pad=5), _c("E-p65", 50, 16, 10, R=1, P=65, rows=(0, 1, 15, 16, 63, 64)),
    _c("E-p66", 50, 17, 3, R=2, P=66, r0=BIG, rows=(0, 63, 64, 65, 66, 67, 130, 131), pad=5),
    # G
    _c("G-min-ld", 3001, 600, 10, R=3, P=3, r0=BIG, scale=-1), _c("G-wide-ld", 601, 200, 10, R=3, P=4, scale=3, pad=5),
    _c("G-tiny", 4, 2, 1, R=4, P=2, scale=-1), _c("G-kf513", 515, 33, 2, R=3, P=3, scale=3),
    # H
    _c("H-fast", 601, 200, 10, fast=True), _c("H-fast-37", 500, 37, 1, r0=BIG, fast=True, pad=5),
    _c("H-fast-scaled", 601, 201, 10, R=3, P=3, scale=-1, fast=True), _c("H-fast-scaled-tiny", 4, 2, 1, R=3, P=2, scale=3, fast=True),
]
IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def czt_fits(c):
    """the contract of pta_gwb_czt_fits, restated"""
    return (c["Nf"] >= 3 and c["npts"] >= 1 and c["i0"] >= 1 and c["Nf"] - 2 + c["npts"] - 2 < FFT_N
            and c["i0"] + c["npts"] - 2 < FFT_N)


def operands(c):
    """everything a call needs besides the shape, reproducible from the case alone: sqrtC [Nf]; w (re, im) [R P, Nf] for a replay;
    scale [R, ld_scale] and ld_scale (or None, 0); rows"""
    Nf, R, P = c["Nf"], c["R"], c["P"]
    rng = np.random.default_rng([Nf, c["npts"], c["i0"], R, P, c["r0"] % 1000])
    sqrtC = rng.uniform(0.5, 2.0, Nf) * 1e-7
    w = rng.standard_normal((2, R * P, Nf))
    scale, ld = None, 0
    if "scale" in c["extras"]:
        ld = Nf + c["extras"]["scale"]
        scale = np.full((R, ld), np.nan)
        scale[:, 1:Nf - 1] = rng.uniform(0.2, 3.0, (R, Nf - 2)) * (1.0 + np.arange(R))[:, None]
    rows = c["extras"].get("rows", tuple(range(R * P)))
    return dict(sqrtC=sqrtC, w=(w[0], w[1]), scale=scale, ld_scale=ld, rows=rows, fast=bool(c["extras"].get("fast")))


_refs = {}


def reference(name, replay=False):
    """gwb_reference's result for the case, computed once per session: drawn on chip (with the case's scale and rng_fast), or the
    replay of operands()["w"] (no scale: the replay entry points take none)"""
    from gwb_reference import gwb_reference
    key = (name, bool(replay))
    if key not in _refs:
        c = BY_NAME[name]
        op = operands(c)
        _refs[key] = gwb_reference(op["sqrtC"], c["Nf"], c["npts"], c["i0"], INV_DT, op["rows"], c["P"], w=op["w"] if replay else None,
                                   seed=SEED, r0=c["r0"], scale=None if replay else op["scale"], fast=op["fast"] and not replay)
    return _refs[key]
