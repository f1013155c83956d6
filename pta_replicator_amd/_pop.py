"""A binned binary population per realisation (ReplicaEngine.set_population): host-side validation and the tables of pta_pop_draw_select
/ pta_pop_theta.  Plain functions of the arrays, so that they run (and are tested) without a GPU, like _cw.py.

The model is the reference's add_gwb_plus_outlier_cws (deterministic.py:565-715) with the Poisson sampling of the cell counts moved in
front of it: per realisation N_b ~ Poisson(number_b), w_b = ((N_b hs2_b) fo_b) T_obs, per frequency bin the outlier_per_bin cells with
the largest w > 0 (ties: the lower cell index) become CW sources, the rest is summed into the free spectrum.  theta then holds
    gwb_log10_hc [R, F]                              0.5 log10(free_spec), the nodes of set_gwb(userSpec=...) = the bin centres
    cw_log10_mc, cw_log10_fgw, cw_log10_dist [R, S]  S = F outlier_per_bin, bin-major, NaN past cw_count [R]
    the five orientation keys [R, S]                 source s from stream (8, s), as set_cw_prior(n_sources=S) draws them
    pop_cell [R, S] int32, pop_number [R, S]         labels: the original cell index (-1 past the count) and the count N of each source
"""
import numpy as np

from . import _cw, _population
from ._hyper import SPEC_KEY, _xp

LABEL_KEYS = ("pop_cell", "pop_number")   # labels of theta, no parameters: generate() and the statistics skip them
KMAX, FMAX = 128, 64                      # PTA_POP_KMAX, PTA_POP_FMAX
INVERSION_BELOW, NORMAL_FROM = 10.0, float(1 << 20)   # PTA_POP_INVERSION_BELOW, PTA_POP_NORMAL_FROM (csrc/pta_pop.h)


def strip_labels(theta):
    """theta without the population's label keys"""
    if any(k in theta for k in LABEL_KEYS):
        return {k: v for k, v in theta.items() if k not in LABEL_KEYS}
    return theta


def regime(number):
    """pta_pop_regime of every rate: 0 none, 1 inversion, 2 PTRS, 3 normal"""
    lam = np.asarray(number, dtype=np.float64)
    return np.where(lam >= NORMAL_FROM, 3, np.where(lam >= INVERSION_BELOW, 2, np.where(lam > 0, 1, 0))).astype(np.int32)


def make_tables(vals, number, fobs, T_obs, outlier_per_bin=100, population=None):
    """validated set_population() arguments -> the host tables: the cells inside the bin edges sorted by (frequency bin, regime of the
    rate, rate, original index), cell_ptr [F + 1], per sorted cell number / hs2 / fo / orig, per original cell log10_mc [Msun] /
    log10_fo [Hz] / log10_dl [Mpc] as NumPy computes them (the device only gathers these), and f_centers [F]."""
    vals = np.asarray(vals, dtype=np.float64)
    number = np.asarray(number, dtype=np.float64)
    fobs = np.asarray(fobs, dtype=np.float64)
    if vals.ndim != 2 or vals.shape[0] != 4 or vals.shape[1] < 1:
        raise ValueError(f"set_population: vals must be [4, B] (Mtot, q, z, f_obs), got shape {vals.shape}")
    B = vals.shape[1]
    if B >= 1 << 31:
        raise ValueError(f"set_population: {B} cells do not fit the 32-bit cell index")
    if number.shape != (B,):
        raise ValueError(f"set_population: number must be [B] = ({B},), got shape {number.shape}")
    if fobs.ndim != 1 or fobs.size < 2:
        raise ValueError(f"set_population: fobs must be the F + 1 bin edges, got shape {fobs.shape}")
    F = fobs.size - 1
    if F > FMAX:
        raise ValueError(f"set_population: at most {FMAX} frequency bins, got F = {F}")
    if not np.all(np.isfinite(fobs)) or np.any(fobs <= 0) or np.any(np.diff(fobs) <= 0):
        raise ValueError("set_population: fobs must be finite, positive and increasing")
    if isinstance(outlier_per_bin, bool) or not isinstance(outlier_per_bin, (int, np.integer)) or not 1 <= outlier_per_bin <= KMAX:
        raise ValueError(f"set_population: outlier_per_bin must be an integer in 1 .. {KMAX}, got {outlier_per_bin!r}")
    T_obs = float(T_obs)
    if not np.isfinite(T_obs) or T_obs <= 0:
        raise ValueError("set_population: T_obs must be finite and > 0 [s]")
    if not np.all(np.isfinite(number)) or np.any(number < 0):
        raise ValueError("set_population: number must be finite and >= 0")
    if not np.all(np.isfinite(vals)):
        raise ValueError("set_population: vals must be finite")
    mc, dl, hs, fo = _population.cell_quantities(vals, population)
    hs2 = hs ** 2
    k_of = np.digitize(fo, fobs) - 1
    inside = (k_of >= 0) & (k_of < F)   # cells outside the edges are dropped, as in the reference
    reg = regime(number)
    order = np.lexsort((np.arange(B), number, reg, k_of))
    order = order[inside[order]]
    cell_ptr = np.searchsorted(k_of[order], np.arange(F + 1), side="left").astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        labels = dict(log10_mc=np.log10(mc / _population.MSOL_CGS), log10_fo=np.log10(fo), log10_dl=np.log10(dl / _population.PC_CGS / 1e6))
    return dict(B=B, F=F, k=int(outlier_per_bin), T_obs=T_obs, fobs=fobs, f_centers=_population.f_centers(fobs), cell_ptr=cell_ptr,
                number=np.ascontiguousarray(number[order]), hs2=np.ascontiguousarray(hs2[order]), fo=np.ascontiguousarray(fo[order]),
                orig=order.astype(np.int32), **labels)


def check_engine(tab, gw, cw, cw_prior, prior, td):
    """refuse a population the engine's configuration cannot carry: its keys go to the free-spectrum GWB and to the CW catalogue."""
    if td:
        raise ValueError("set_population: not available in TD mode (the dense factors are built for one spectrum)")
    if gw is None or gw.get("userSpec") is None:
        raise ValueError("set_population: needs set_gwb(..., userSpec=U) with the bin centres of fobs as node frequencies")
    U = np.asarray(gw["userSpec"], dtype=np.float64)
    fc = tab["f_centers"]
    if U.ndim != 2 or U.shape[0] != len(fc) or U.shape[1] != 2 or not np.all(np.abs(U[:, 0] - fc) <= 1e-12 * fc):
        raise ValueError("set_population: the node frequencies of set_gwb's userSpec must equal the bin centres of fobs "
                         "(_population.f_centers(fobs), relative 1e-12), in their order")
    if cw is None:
        raise ValueError("set_population: no per-realisation CW configured (set_cw)")
    if cw_prior is not None:
        raise ValueError("set_population: cannot be combined with set_cw_prior (both define the cw_* keys)")
    if prior is not None and SPEC_KEY in prior:
        raise ValueError(f"set_population: cannot be combined with a {SPEC_KEY} prior (both define the key)")


def check_counts(counts, R, B):
    """counts of population_theta validated: [R, B] finite and >= 0 (NumPy or tensor; returned as given)"""
    c = counts if isinstance(counts, np.ndarray) or hasattr(counts, "device") else np.asarray(counts, dtype=np.float64)
    if tuple(c.shape) != (R, B):
        raise ValueError(f"population_theta: counts must be [R, B] = {(R, B)}, got shape {tuple(c.shape)}")
    if not bool(_xp(c).isfinite(c).all()) or bool((c < 0).any()):
        raise ValueError("population_theta: counts must be finite and >= 0")
    return c


def orientation_prior(P, S):
    """the set_cw_prior(n_sources=S) dict whose five orientation boxes are the defaults; its three source boxes are placeholders that
    the population's own columns replace"""
    return _cw.make_prior(P, n_sources=S, log10_mc=(0.0, 0.0), log10_fgw=(0.0, 0.0), log10_dist=(0.0, 0.0))
