"""Per-realisation hyperparameters (theta) of ReplicaEngine's throughput mode: host-side validation and the column layout of
sampled theta.  Plain functions of the configuration and the arrays, so that they run (and are tested) without a GPU.

theta is a dict with any subset of
    gwb_log10_A, gwb_gamma   [R]      GWB amplitude / spectral index of realisation r0 + r
    rn_log10_A, rn_gamma     [R, P]   red-noise amplitude / spectral index of pulsar a in realisation r0 + r
    gwb_log10_hc             [R, M]   log10 characteristic strain of realisation r0 + r at the M nodes of the configured userSpec
    gwb_clm                  [R, (lmax+1)^2]   angular power coefficients c_lm of realisation r0 + r, column k = l^2 + m + l
as NumPy arrays or torch tensors.  A key that is not given keeps its configured value.  NaN in rn_log10_A means "this pulsar as
configured" (amplitude and index); a pulsar configured without red noise keeps none whatever its entries say.
"""
import numpy as np

GWB_KEYS = ("gwb_log10_A", "gwb_gamma")
RN_KEYS = ("rn_log10_A", "rn_gamma")
KEYS = GWB_KEYS + RN_KEYS
# the per-realisation GWB spectrum of an engine configured with set_gwb(userSpec=U [M, 2]): row r replaces log10(U[:, 1]), column j
# belongs to row j of U as given.  Kept beside KEYS: it is no column of the pta_hyper_uniform table (its nodes are drawn from
# stream (7, SPEC_FIELD), pair = node)
SPEC_KEY = "gwb_log10_hc"
SPEC_FIELD = 1
SPEC_MAX_NODES = 4096   # PTA_GWB_SPEC_MMAX: the nodes of one realisation are staged in LDS
# the per-realisation angular power distribution of an engine configured with set_gwb(lmax=L >= 1): row r replaces the configured clm
# (ORF_r = 2 sum_k clm[r, k] basis[k], column order of correlated_basis).  Its l >= 1 columns are drawn from stream (7, CLM_FIELD),
# pair = column; column 0 (c_00) stays as configured
CLM_KEY = "gwb_clm"
CLM_FIELD = 2
ORF_INFO_KEY = "gwb_orf_info"   # label of sampled theta: info [R] of pta_gwb_orf_factor (0 = positive definite); no parameter
ALL_KEYS = KEYS + (SPEC_KEY, CLM_KEY)


def n_columns(P):
    """parameters per realisation drawn by pta_hyper_uniform: [gwb_log10_A, gwb_gamma, rn_log10_A x P, rn_gamma x P]."""
    return 2 + 2 * P


def columns(P):
    """column range of every key in the [R, n_columns(P)] theta table that pta_hyper_uniform fills (stream kind 7, pair = column)."""
    return {"gwb_log10_A": (0, 1), "gwb_gamma": (1, 2), "rn_log10_A": (2, 2 + P), "rn_gamma": (2 + P, 2 + 2 * P)}


def check_config(keys, gw, rn, gwb_mode):
    """refuse theta keys the configuration cannot honour (before anything is launched)."""
    keys = set(keys)
    unknown = keys - set(ALL_KEYS)
    if unknown:
        raise ValueError(f"theta: unknown keys {sorted(unknown)} (expected a subset of {list(ALL_KEYS)})")
    if SPEC_KEY in keys and gw is None:
        raise ValueError("theta: a GWB spectrum given but no GWB is configured (set_gwb)")
    if keys & set(GWB_KEYS):
        if gw is None:
            raise ValueError("theta: GWB parameters given but no GWB is configured (set_gwb)")
        if gw.get("userSpec") is not None:
            raise ValueError("theta: GWB parameters cannot rescale a userSpec spectrum (only the power law has (log10_A, gamma))")
        if gwb_mode == "grid":
            raise ValueError("theta: GWB parameters need gwb_mode='fourier' (the 'grid' factor is built for one spectrum)")
    if SPEC_KEY in keys:
        if gw.get("userSpec") is None:
            raise ValueError(f"theta: {SPEC_KEY} needs a GWB configured with a userSpec spectrum (its frequency column fixes the nodes)")
        if keys & set(GWB_KEYS):
            raise ValueError("theta: GWB parameters cannot rescale a userSpec spectrum (only the power law has (log10_A, gamma))")
        if gwb_mode == "grid":
            raise ValueError(f"theta: {SPEC_KEY} needs gwb_mode='fourier' (the 'grid' factor is built for one spectrum)")
        spec_nodes(gw["userSpec"])
    if CLM_KEY in keys:
        if gw is None:
            raise ValueError(f"theta: {CLM_KEY} given but no GWB is configured (set_gwb)")
        if gw.get("no_correlations"):
            raise ValueError(f"theta: {CLM_KEY} needs a correlated GWB (set_gwb(no_correlations=True) has no ORF to shape)")
        if n_lm(gw) is None:
            raise ValueError(f"theta: {CLM_KEY} needs a GWB configured with set_gwb(lmax=L), L >= 1 (lmax fixes the columns; at lmax = 0 the "
                             "only coefficient is the amplitude)")
        if gwb_mode == "grid":
            raise ValueError(f"theta: {CLM_KEY} needs gwb_mode='fourier' (the 'grid' path mixes with the one configured ORF factor)")
    if keys & set(RN_KEYS) and rn is None:
        raise ValueError("theta: red-noise parameters given but no red noise is configured (set_red_noise)")


def n_lm(gw):
    """(lmax + 1)^2 of a GWB configuration that can carry gwb_clm per realisation (lmax >= 1, correlated), else None"""
    if gw is None or gw.get("no_correlations") or int(gw.get("lmax") or 0) < 1:
        return None
    return (int(gw["lmax"]) + 1) ** 2


def configured_clm(gw):
    """the configured clm [n_lm] (the first n_lm entries, as the reference's sum reads them)"""
    n = n_lm(gw)
    c = np.asarray(gw["clm"], dtype=np.float64).ravel()
    if len(c) < n:
        raise IndexError(f"clm has {len(c)} coefficients but lmax={gw['lmax']} needs {n}")
    return c[:n].copy()


def spec_nodes(userSpec):
    """(order [M], xp [M]) of a userSpec [M, 2]: the stable sort by frequency that red_noise.gwb_spectrum_hcf applies and log10 of the
    sorted node frequencies.  Refuses what a per-realisation spectrum cannot be interpolated on."""
    U = np.asarray(userSpec, dtype=np.float64)
    if U.ndim != 2 or U.shape[1] != 2 or U.shape[0] < 2:
        raise ValueError(f"userSpec: a per-realisation spectrum needs at least 2 node frequencies ([M, 2], M >= 2), got shape {U.shape}")
    if U.shape[0] > SPEC_MAX_NODES:
        raise ValueError(f"userSpec: a per-realisation spectrum takes at most {SPEC_MAX_NODES} node frequencies, got {U.shape[0]}")
    order = np.argsort(U[:, 0], kind="mergesort")
    f = U[order, 0]
    if not np.all(np.isfinite(f)) or np.any(f <= 0) or np.any(np.diff(f) <= 0):
        raise ValueError("userSpec: a per-realisation spectrum needs finite, positive and distinct node frequencies")
    if not np.all(np.isfinite(U[:, 1])) or np.any(U[:, 1] <= 0):   # the configured hc is the divisor of the per-realisation scale
        raise ValueError("userSpec: a per-realisation spectrum needs finite, positive hc at every node")
    return order, np.log10(f)


def spec_tables(f, xp):
    """(seg int32 [n], dx [n], dxp [n]) for frequencies f and sorted node abscissae xp = log10(node frequencies): what numpy.interp
    derives from the abscissae alone.  seg = j with xp[j] <= log10 f < xp[j + 1], dx = log10 f - xp[j], dxp = xp[j + 1] - xp[j];
    dxp = 0 marks a frequency that takes node seg itself: below the first node (seg 0), at or above the last (seg M - 1), or
    exactly on a node.  pta_gwb_hcf_user (csrc/pta_hyper.h) and spec_eval evaluate a spectrum from them."""
    x = np.log10(np.asarray(f, dtype=np.float64))
    xp = np.asarray(xp, dtype=np.float64)
    M = len(xp)
    j = np.searchsorted(xp, x, side="right") - 1
    seg = np.clip(j, 0, M - 1)
    dx = x - xp[seg]
    inside = (j >= 0) & (j < M - 1) & (dx != 0.0)
    dxp = np.where(inside, xp[np.minimum(seg + 1, M - 1)] - xp[seg], 0.0)
    return seg.astype(np.int32), np.where(inside, dx, 0.0), dxp


def spec_eval(tables, fp):
    """hc [..., n] of spectra with sorted node values fp [..., M] (log10 hc) at the frequencies of `tables` (spec_tables): NumPy form
    of pta_gwb_hcf_user, the same operations in the same order."""
    seg, dx, dxp = tables
    fp = np.asarray(fp, dtype=np.float64)
    lo = fp[..., seg]
    hi = fp[..., np.minimum(seg + 1, fp.shape[-1] - 1)]
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(dxp != 0.0, (hi - lo) / dxp * dx + lo, lo)
    return 10.0 ** y


def _n_nodes(gw):
    return None if gw is None or gw.get("userSpec") is None else int(np.shape(gw["userSpec"])[0])


def _xp(x):
    """the array module of x: torch for tensors, else NumPy."""
    if isinstance(x, np.ndarray) or not hasattr(x, "device"):
        return np
    import torch
    return torch


def _as_array(name, x):
    if isinstance(x, np.ndarray) or hasattr(x, "device"):
        return x
    try:
        return np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"theta[{name!r}]: expected an array of numbers") from None


def check_theta(theta, R, P, gw, rn, gwb_mode, check_values=True):
    """validate theta for R realisations of a P-pulsar array against the configuration; returns {key: array} (the caller's arrays,
    unconverted).  check_values=False skips the value checks (theta drawn by pta_hyper_uniform: finite by construction)."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    check_config(theta.keys(), gw, rn, gwb_mode)
    return _check_arrays(theta, R, P, rn, check_values, _n_nodes(gw), n_lm(gw))


def check_theta_os(theta, R, P, rn, gwb_auto, check_values=True, gw=None):
    """validate theta as the noise model of the optimal statistic (optimal_statistic(theta=...), generate_os(matched=True)): keys,
    shapes and NaN rules of check_theta, without its gwb_mode restriction (the OS does not care how the GWB was generated).  GWB
    keys are refused when the OS was prepared without the GWB auto-term (gwb_auto false); cw_* keys are ignored (a deterministic
    source is not part of the noise model, and so is gwb_clm: the auto-term stays the isotropic one).  gw: the engine's GWB configuration; given, the spectrum key gwb_log10_hc is accepted too
    (its nodes are the configured userSpec's; left out, as by the likelihood grid, the key is unknown).  Returns {key: array} of the
    GWB / red-noise keys."""
    from . import _chrom, _cproc, _cw, _wn_hyper
    _wn_hyper.refuse_noise_model(theta)   # the matched statistics hold white noise fixed: said so, instead of "unknown keys"
    _chrom.refuse_noise_model(theta)      # and carry no chromatic term
    _cproc.refuse_noise_model(theta)
    theta, _ = _cw.split(theta)
    if gw is not None:
        theta = {k: v for k, v in theta.items() if k not in (CLM_KEY, ORF_INFO_KEY)}
    known = KEYS if gw is None else KEYS + (SPEC_KEY,)
    unknown = set(theta) - set(known)
    if unknown:
        raise ValueError(f"theta: unknown keys {sorted(unknown)} (expected a subset of {list(known)})")
    if set(theta) & set(GWB_KEYS + (SPEC_KEY,)) and not gwb_auto:
        raise ValueError("theta: GWB parameters given but the optimal statistic was prepared without the GWB auto-term (gwb_auto)")
    if SPEC_KEY in theta:
        if gw.get("userSpec") is None:
            raise ValueError(f"theta: {SPEC_KEY} needs a GWB configured with a userSpec spectrum (its frequency column fixes the nodes)")
        if set(theta) & set(GWB_KEYS):
            raise ValueError("theta: GWB parameters cannot rescale a userSpec spectrum (only the power law has (log10_A, gamma))")
        spec_nodes(gw["userSpec"])
    if set(theta) & set(RN_KEYS) and rn is None:
        raise ValueError("theta: red-noise parameters given but no red noise is configured (set_red_noise)")
    return _check_arrays(theta, R, P, rn, check_values, _n_nodes(gw))


def _check_arrays(theta, R, P, rn, check_values, M=None, L=None):
    """shapes and values of theta's GWB / red-noise arrays (keys already checked against the configuration); M: nodes of the
    configured userSpec (the columns of gwb_log10_hc); L: (lmax + 1)^2 of the configured GWB (the columns of gwb_clm)."""
    out = {}
    for k, v in theta.items():
        v = _as_array(k, v)
        want = (R,) if k in GWB_KEYS else (R, M) if k == SPEC_KEY else (R, L) if k == CLM_KEY else (R, P)
        if tuple(v.shape) != want:
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {want}")
        out[k] = v
    if not check_values:
        return out
    for k in GWB_KEYS + (SPEC_KEY, CLM_KEY):
        if k in out and not bool(_xp(out[k]).isfinite(out[k]).all()):
            raise ValueError(f"theta[{k!r}]: non-finite values")
    if "rn_log10_A" in out:
        a = out["rn_log10_A"]
        if bool(_xp(a).isinf(a).any()):
            raise ValueError("theta['rn_log10_A']: infinite values (NaN alone means 'as configured')")
    if "rn_gamma" in out:
        g = out["rn_gamma"]
        if "rn_log10_A" in out:
            a = out["rn_log10_A"]
            sampled = ~_xp(a).isnan(a)
        else:   # index sampled, amplitude as configured: every pulsar that has red noise needs a finite index
            sampled = np.broadcast_to(~np.isnan(configured_rn(rn)[0]), (R, P))
        xp = _xp(g)
        if xp is np:
            sampled = _host(sampled)
        elif _xp(sampled) is np:
            sampled = xp.as_tensor(np.ascontiguousarray(sampled), device=g.device)
        else:
            sampled = sampled.to(g.device)
        if bool((xp.isinf(g) | (xp.isnan(g) & sampled)).any()):
            raise ValueError("theta['rn_gamma']: non-finite values where the amplitude is sampled")
    return out


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def configured_rn(rn):
    """configured (log10_A, gamma) of every pulsar, NaN where it has no red noise."""
    lA = np.array([np.nan if (a is None or g is None) else float(a) for a, g in zip(rn["A"], rn["g"])])
    g = np.array([np.nan if (a is None or g_ is None) else float(g_) for a, g_ in zip(rn["A"], rn["g"])])
    return lA, g


def prior_bounds(prior, P):
    """lo, hi [n_columns(P)] of pta_hyper_uniform for a prior dict {key: (lo [n], hi [n])}; columns not sampled are [0, 0)."""
    lo, hi = np.zeros(n_columns(P)), np.zeros(n_columns(P))
    cols = columns(P)
    for k, (l, h) in prior.items():
        if k in (SPEC_KEY, CLM_KEY):   # their own tables: spec_bounds, clm_bounds
            continue
        c0, c1 = cols[k]
        lo[c0:c1], hi[c0:c1] = l, h
    return lo, hi


def spec_bounds(prior):
    """lo, hi [M] of pta_hyper_uniform_field(field = SPEC_FIELD) for the gwb_log10_hc boxes of a prior dict: column j = node j of the
    userSpec as given; None when the spectrum is not sampled."""
    return prior.get(SPEC_KEY)


def clm_bounds(prior, gw):
    """lo, hi [n_lm] of pta_hyper_uniform_field(field = CLM_FIELD) for the gwb_clm boxes of a prior dict: pair j = column j of gwb_clm;
    column 0 is the box [c_00, c_00) of the configured c_00 (lo + 0 u = c_00 exactly); None when clm is not sampled."""
    if CLM_KEY not in prior:
        return None
    c00 = configured_clm(gw)[0]
    l, h = prior[CLM_KEY]
    return np.concatenate([[c00], l]), np.concatenate([[c00], h])


def make_prior(P, M=None, L=None, **boxes):
    """validated {key: (lo [n], hi [n])} of set_hyper_prior: GWB keys take (lo, hi); RN keys (lo, hi) for all pulsars or [P, 2];
    gwb_log10_hc (lo, hi) for all M nodes of the configured userSpec or [M, 2] (M None: no userSpec is configured); gwb_clm (lo, hi)
    for all L - 1 coefficients with l >= 1 or [L - 1, 2], L = (lmax + 1)^2 (None: no lmax >= 1 is configured)."""
    prior = {}
    for k, box in boxes.items():
        if box is None:
            continue
        if k not in ALL_KEYS:
            raise ValueError(f"set_hyper_prior: unknown parameter {k!r} (expected one of {list(ALL_KEYS)})")
        if k == SPEC_KEY and M is None:
            raise ValueError(f"set_hyper_prior: {k} needs a GWB configured with a userSpec spectrum (its frequency column fixes the nodes)")
        if k == CLM_KEY and L is None:
            raise ValueError(f"set_hyper_prior: {k} needs a correlated GWB configured with set_gwb(lmax=L), L >= 1")
        b = np.asarray(box, dtype=np.float64)
        n = 1 if k in GWB_KEYS else M if k == SPEC_KEY else L - 1 if k == CLM_KEY else P
        if b.shape == (2,):
            b = np.broadcast_to(b, (n, 2))
        if b.shape != (n, 2):
            raise ValueError(f"set_hyper_prior: {k} must be (lo, hi){'' if n == 1 else f' or [{n}, 2]'}, got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or np.any(b[:, 1] < b[:, 0]):
            raise ValueError(f"set_hyper_prior: {k} needs finite bounds with lo <= hi")
        prior[k] = (b[:, 0].copy(), b[:, 1].copy())
    if not prior:
        raise ValueError("set_hyper_prior: no parameter given")
    return prior
