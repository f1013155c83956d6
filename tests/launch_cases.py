"""The shapes at which every kernel instance that a host launcher picks from the size of a launch is reached.

The launchers of the table below choose a kernel instance, or the work of one workgroup, from R, P, G or the number of tiles; each
promises that the choice only regroups realisations (grid points, tiles) and that no output value depends on it.  The GPU tests import
their shapes from here; tests/test_launch_cases.py asks the library's pta_*_plan entries (no device call) that every case reaches
the instance it names and that together the cases cover every instance, so a retuned threshold fails there, on the CPU, instead of
silently sending the GPU tests down the small-launch branch again.

A case is {"launcher", "sizes", "expect"}: `sizes` are the arguments of the launcher's pta_*_plan entry in order, `expect` the plan
values the case exists for (a subset of the plan's keys)."""
import numpy as np


def plan(launcher, *sizes):
    """the launcher's own choice for these sizes (pta_replicator_amd._lib.launch_plan)"""
    from pta_replicator_amd import _lib
    return _lib.launch_plan(launcher, *sizes)


def case(launcher, sizes, **expect):
    return {"launcher": launcher, "sizes": tuple(int(v) for v in sizes), "expect": expect}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- pta_os_project: rw = 2 -------------------------------------
# rw = 2 from cdiv(R, 128) * P >= 1024: 1024 pulsars reach it at every R.  The launch that takes the other branch is the same
# realisations over a window of 8 of the pulsars (psr_off shifted), which holds four of the long ones.
OS_P = 1024
OS_LONG = {0: 130, 1017: 65, 1019: 130, 1020: 301, 1023: 257}   # pulsars of more than one K chunk of 64 TOAs: the prefetch runs with two tiles
OS_R = (1, 17, 130)
OS_C = (2, 28, 40, 64)
OS_WINDOW = (1016, 8)                                            # (first pulsar, pulsars) of the small launch


def os_counts():
    counts = np.random.default_rng(1024).integers(1, 41, OS_P)
    for a, n in OS_LONG.items():
        counts[a] = n
    return counts


def os_windows(R):
    """(first realisation, count) of the small launches: the first realisations and the last ones (of a partial tile)"""
    return sorted({(0, min(2, R)), (max(0, R - 3), min(3, R))})


OS_CASES = [case("pta_os_project", (C, OS_P, R), rw=2, ct=cdiv(C, 16)) for C in OS_C for R in OS_R]
OS_CASES += [case("pta_os_project", (C, OS_WINDOW[1], n), rw=1, ct=cdiv(C, 16)) for C in OS_C for n in (1, 2, 3)]

# ---------------------------------------------------------------- pta_lnl_apply: g_per and KT --------------------------------
# g_per = clamp(G * P * cdiv(R, 128) / 4096, 1, 16) grid points per workgroup.  sub_g / sub_r: the grid points and realisations that are
# recomputed in a launch of their own (g_per = 1), with those of the short last group and of the partial last tile among them.
LNL_GROUPS = [
    dict(P=64, K=29, G=130, R=1, g_per=2, sub_g=(0, 1, 2, 129), sub_r=(0,)),
    dict(P=32, K=40, G=130, R=300, g_per=3, sub_g=(0, 1, 2, 3, 128, 129), sub_r=(0, 127, 128, 297, 298, 299)),   # 44 groups, the last with 1
    dict(P=128, K=5, G=515, R=1, g_per=16, sub_g=(0, 15, 16, 511, 512, 513, 514), sub_r=(0,)),                 # 33 groups, the last with 3
]
LNL_K_FIRST = (2, 29, 88, 128)              # test_factor_apply_vs_numpy: KT = 1, 2, 6, 8
LNL_K_MORE = (40, 64, 65, 80, 100, 112)     # KT = 3, 4, 5, 5, 7, 7
LNL_KT_SHAPE = dict(P=2, G=5, R=17)

LNL_CASES = [case("pta_lnl_apply", (c["P"], c["K"], c["G"], c["R"]), kt=cdiv(c["K"], 16), g_per=c["g_per"]) for c in LNL_GROUPS]
LNL_CASES += [case("pta_lnl_apply", (c["P"], c["K"], len(c["sub_g"]), len(c["sub_r"])), kt=cdiv(c["K"], 16), g_per=1) for c in LNL_GROUPS]
LNL_CASES += [case("pta_lnl_apply", (LNL_KT_SHAPE["P"], K, LNL_KT_SHAPE["G"], LNL_KT_SHAPE["R"]), kt=cdiv(K, 16), g_per=1)
              for K in LNL_K_FIRST + LNL_K_MORE]

# ---------------------------------------------------------------- pta_fstat_project: the six tiles ---------------------------
FSTAT_PROJECT_R = 1000
FSTAT_PROJECT_LARGE = [(64, 512), (33, 512), (256, 64), (256, 30)]        # (P, C) of test_fstat_project_large_launch_tiles
FSTAT_PROJECT_TILES = {(64, 512): (128, 128), (33, 512): (64, 128), (256, 64): (128, 64), (256, 30): (128, 32)}
FSTAT_PROJECT_CASES = [case("pta_fstat_project", (C, P, FSTAT_PROJECT_R), bm=FSTAT_PROJECT_TILES[P, C][0], bn=FSTAT_PROJECT_TILES[P, C][1])
                       for P, C in FSTAT_PROJECT_LARGE]
# the launch of 3 realisations the same test compares with: 64 rows, and 64 columns unless C <= 32
FSTAT_PROJECT_CASES += [case("pta_fstat_project", (C, P, 3), bm=64, bn=32 if C <= 32 else 64) for P, C in FSTAT_PROJECT_LARGE]

# ---------------------------------------------------------------- pta_gwb_mix_batched: tiles per workgroup --------------------
# tpw = ntile when R >= 512 or ntile <= 4, else 4; 300 samples are 5 tiles of 64: below 512 realisations the second workgroup of a
# realisation takes tile 4 and leaves its loop at tile 5 (the skipped tail), from 512 on one workgroup walks all five.
MIX_TILE = 64
MIX_P = (3, 17, 40, 49, 80)                 # nta = ceil(P / 16) = 1 .. 5: every k_gwb_mix_batched<nta>
MIX_NPTS = 300
MIX_R = (511, 512)
MIX_SMALL_R = 3
MIX_CASES = [case("pta_gwb_mix_batched", (P, 511, MIX_NPTS, 0), nta=cdiv(P, 16), tpw=4, grid_x=2) for P in MIX_P]
MIX_CASES += [case("pta_gwb_mix_batched", (P, 512, MIX_NPTS, 0), nta=cdiv(P, 16), tpw=5, grid_x=1) for P in MIX_P]
MIX_CASES += [case("pta_gwb_mix_batched", (P, MIX_SMALL_R, MIX_NPTS, 0), nta=cdiv(P, 16), tpw=4, grid_x=2) for P in MIX_P]

# ---------------------------------------------------------------- the sky statistics: rchunk and KS ---------------------------
# rchunk = ceil(R / nz), nz = min(4096 / (nst * njb), (R + 7) / 8, 65535): a chunk is 8 realisations (or all of them) unless the sky
# grid alone has more than 512 workgroups.  RB realisations share one scan of the maxima: rchunk % RB != 0 ends a chunk part-way.
SKY_RB = {"pta_fstat_fe": 8, "pta_bwm_stat": 4}
# (P, J, S, R): rchunk, and the windows (first realisation, count <= 8) recomputed in a launch of their own (one workgroup walks them)
SKY_CHUNK = {
    "pta_fstat_fe": [dict(P=5, J=17, S=2560, R=300, rchunk=9, windows=((7, 4), (296, 4))),          # 34 chunks of 9, the last of 3
                     dict(P=23, J=11, S=100, R=37, rchunk=8, windows=((5, 4), (33, 4))),
                     dict(P=6, J=9, S=65, R=7, rchunk=7, windows=((4, 3),))],                         # nz = 1
    "pta_bwm_stat": [dict(P=5, J=3, S=7675, R=300, rchunk=9, windows=((7, 4), (296, 4))),           # 120 sky tiles, the last partial
                     dict(P=23, J=11, S=100, R=37, rchunk=8, windows=((5, 4), (33, 4))),
                     dict(P=6, J=17, S=65, R=7, rchunk=7, windows=((4, 3),))],
}
# one P per KS = ceil(P / 4) = 1 .. 32: full steps (P = 4 k) and steps with one pulsar (P = 4 k + 1) in turn; P = 2, 3: the smallest
SKY_KS_P = (2, 3, 4) + tuple(4 * ks if ks % 2 == 0 else 4 * (ks - 1) + 1 for ks in range(2, 33))
SKY_KS_SHAPE = dict(J=2, S=17, R=3)

SKY_CASES = []
for _name, _cases in SKY_CHUNK.items():
    for _c in _cases:
        SKY_CASES.append(case(_name, (_c["P"], _c["J"], _c["R"], _c["S"]), ks=cdiv(_c["P"], 4), rchunk=_c["rchunk"]))
        SKY_CASES += [case(_name, (_c["P"], _c["J"], n, _c["S"]), ks=cdiv(_c["P"], 4), rchunk=n, ngz=1) for _, n in _c["windows"]]
    SKY_CASES += [case(_name, (P, SKY_KS_SHAPE["J"], SKY_KS_SHAPE["R"], SKY_KS_SHAPE["S"]), ks=cdiv(P, 4), ngz=1) for P in SKY_KS_P]

# ---------------------------------------------------------------- pta_tm_project: m = 1 .. 12 ---------------------------------
TM_M = tuple(range(1, 13))
TM_R = (1, 8, 9, 23)                          # 8 realisations per workgroup: one, a full group, one past it, a partial last group
TM_COUNTS = (1, 255, 256, 257, 700)           # around the 256 threads of a workgroup, and more than two strides
TM_CASES = [case("pta_tm_project", (m, len(TM_COUNTS), R), m=m, grid_y=cdiv(R, 8)) for m in TM_M for R in TM_R]

ALL_CASES = OS_CASES + LNL_CASES + FSTAT_PROJECT_CASES + MIX_CASES + SKY_CASES + TM_CASES
