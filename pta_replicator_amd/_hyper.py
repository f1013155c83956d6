"""Per-realisation hyperparameters (theta) of ReplicaEngine's throughput mode: host-side validation and the column layout of
sampled theta.  Plain functions of the configuration and the arrays, so that they run (and are tested) without a GPU.

theta is a dict with any subset of
    gwb_log10_A, gwb_gamma   [R]      GWB amplitude / spectral index of realisation r0 + r
    rn_log10_A, rn_gamma     [R, P]   red-noise amplitude / spectral index of pulsar a in realisation r0 + r
as NumPy arrays or torch tensors.  A key that is not given keeps its configured value.  NaN in rn_log10_A means "this pulsar as
configured" (amplitude and index); a pulsar configured without red noise keeps none whatever its entries say.
"""
import numpy as np

GWB_KEYS = ("gwb_log10_A", "gwb_gamma")
RN_KEYS = ("rn_log10_A", "rn_gamma")
KEYS = GWB_KEYS + RN_KEYS


def n_columns(P):
    """parameters per realisation drawn by pta_hyper_uniform: [gwb_log10_A, gwb_gamma, rn_log10_A x P, rn_gamma x P]."""
    return 2 + 2 * P


def columns(P):
    """column range of every key in the [R, n_columns(P)] theta table that pta_hyper_uniform fills (stream kind 7, pair = column)."""
    return {"gwb_log10_A": (0, 1), "gwb_gamma": (1, 2), "rn_log10_A": (2, 2 + P), "rn_gamma": (2 + P, 2 + 2 * P)}


def check_config(keys, gw, rn, gwb_mode):
    """refuse theta keys the configuration cannot honour (before anything is launched)."""
    keys = set(keys)
    unknown = keys - set(KEYS)
    if unknown:
        raise ValueError(f"theta: unknown keys {sorted(unknown)} (expected a subset of {list(KEYS)})")
    if keys & set(GWB_KEYS):
        if gw is None:
            raise ValueError("theta: GWB parameters given but no GWB is configured (set_gwb)")
        if gw.get("userSpec") is not None:
            raise ValueError("theta: GWB parameters cannot rescale a userSpec spectrum (only the power law has (log10_A, gamma))")
        if gwb_mode == "grid":
            raise ValueError("theta: GWB parameters need gwb_mode='fourier' (the 'grid' factor is built for one spectrum)")
    if keys & set(RN_KEYS) and rn is None:
        raise ValueError("theta: red-noise parameters given but no red noise is configured (set_red_noise)")


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
    return _check_arrays(theta, R, P, rn, check_values)


def check_theta_os(theta, R, P, rn, gwb_auto, check_values=True):
    """validate theta as the noise model of the optimal statistic (optimal_statistic(theta=...), generate_os(matched=True)): keys,
    shapes and NaN rules of check_theta, without its gwb_mode restriction (the OS does not care how the GWB was generated).  GWB
    keys are refused when the OS was prepared without the GWB auto-term (gwb_auto false); cw_* keys are ignored (a deterministic
    source is not part of the noise model).  Returns {key: array} of the GWB / red-noise keys."""
    from . import _cw
    theta, _ = _cw.split(theta)
    unknown = set(theta) - set(KEYS)
    if unknown:
        raise ValueError(f"theta: unknown keys {sorted(unknown)} (expected a subset of {list(KEYS)})")
    if set(theta) & set(GWB_KEYS) and not gwb_auto:
        raise ValueError("theta: GWB parameters given but the optimal statistic was prepared without the GWB auto-term (gwb_auto)")
    if set(theta) & set(RN_KEYS) and rn is None:
        raise ValueError("theta: red-noise parameters given but no red noise is configured (set_red_noise)")
    return _check_arrays(theta, R, P, rn, check_values)


def _check_arrays(theta, R, P, rn, check_values):
    """shapes and values of theta's GWB / red-noise arrays (keys already checked against the configuration)."""
    out = {}
    for k, v in theta.items():
        v = _as_array(k, v)
        want = (R,) if k in GWB_KEYS else (R, P)
        if tuple(v.shape) != want:
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {want}")
        out[k] = v
    if not check_values:
        return out
    for k in GWB_KEYS:
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
        c0, c1 = cols[k]
        lo[c0:c1], hi[c0:c1] = l, h
    return lo, hi


def make_prior(P, **boxes):
    """validated {key: (lo [n], hi [n])} of set_hyper_prior: GWB keys take (lo, hi); RN keys (lo, hi) for all pulsars or [P, 2]."""
    prior = {}
    for k, box in boxes.items():
        if box is None:
            continue
        if k not in KEYS:
            raise ValueError(f"set_hyper_prior: unknown parameter {k!r} (expected one of {list(KEYS)})")
        b = np.asarray(box, dtype=np.float64)
        n = 1 if k in GWB_KEYS else P
        if b.shape == (2,):
            b = np.broadcast_to(b, (n, 2))
        if b.shape != (n, 2):
            raise ValueError(f"set_hyper_prior: {k} must be (lo, hi){'' if n == 1 else f' or [{P}, 2]'}, got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or np.any(b[:, 1] < b[:, 0]):
            raise ValueError(f"set_hyper_prior: {k} needs finite bounds with lo <= hi")
        prior[k] = (b[:, 0].copy(), b[:, 1].copy())
    if not prior:
        raise ValueError("set_hyper_prior: no parameter given")
    return prior
