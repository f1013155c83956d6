"""White-noise parameters per realisation (theta's wn_* keys) of ReplicaEngine's throughput mode: the keys, the groups they address,
host-side validation and the prior boxes.  Plain functions of the configuration and the arrays, so that they run (and are tested)
without a GPU, like _cw.py and _bwm.py.

A white-noise group is a (pulsar, backend flag) pair of set_white_noise(..., flags=), the pulsar itself when flags is None; groups
are ordered pulsar-major, flags in the order given.  ECORR groups are built the same way from set_jitter; a pulsar whose log10_ecorr
is None has none.  theta may hold, next to the keys of _hyper, _cw and _bwm,
    wn_efac, wn_log10_equad   [R, G_wn]
    wn_log10_ecorr            [R, G_ec]
as NumPy arrays or torch tensors: each entry replaces the configured value of its group for realisation r0 + r, NaN = as
configured; a key that is not given leaves its parameter as configured.  The semantics per realisation are the reference's
(white_noise.py:105-109, :182) with the deviates generate() draws.

Out of scope: TD mode, wn_mode "single", per-TOA parameters, and every statistic whose noise model would have to follow them.
"""
import numpy as np

from ._hyper import _as_array, _xp

EFAC_KEY, EQUAD_KEY, ECORR_KEY = "wn_efac", "wn_log10_equad", "wn_log10_ecorr"
WN_KEYS = (EFAC_KEY, EQUAD_KEY)     # the EFAC / EQUAD term: columns = white-noise groups
KEYS = WN_KEYS + (ECORR_KEY,)       # ECORR_KEY: columns = ECORR groups
# prior draws: pta_hyper_uniform_field on stream (7, FIELD[key]), pair = group (fields 1 and 2: _hyper.SPEC_FIELD, _hyper.CLM_FIELD)
FIELD = {EFAC_KEY: 3, EQUAD_KEY: 4, ECORR_KEY: 5}
GMAX = 16   # PTA_WN_HYPER_GMAX: groups of one pulsar (of either kind) whose amplitude rows pta_engine_wn_add stages


def split(theta):
    """(rest, wn): the white-noise keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    wn = {k: v for k, v in theta.items() if k in KEYS}
    rest = {k: v for k, v in theta.items() if k not in KEYS}
    return rest, wn


def has_keys(det):
    """True if a dict of validated keys (the second member of ReplicaEngine._theta_parts) holds white-noise keys."""
    return bool(det) and any(k in det for k in KEYS)


def has_wn(det):
    return bool(det) and any(k in det for k in WN_KEYS)


def has_ecorr(det):
    return bool(det) and ECORR_KEY in det


def _pick(val, a, P):
    if val is None or np.isscalar(val):
        return val
    if len(val) != P:
        raise ValueError(f"expected a scalar or one entry per pulsar ({P}), got {len(val)}")
    return val[a]


def _pick_flags(flags, a, P):
    if flags is None:
        return None
    if len(flags) != P:
        raise ValueError("flags must be a per-pulsar list of flag lists")
    return flags[a]


def wn_groups(P, wn_conf):
    """[(pulsar index, flag or None)] of a set_white_noise configuration (None: not configured -> [])."""
    if wn_conf is None:
        return []
    out = []
    for a in range(P):
        flags = _pick_flags(wn_conf["flags"], a, P)
        out += [(a, None)] if flags is None else [(a, f) for f in flags]
    return out


def ecorr_groups(P, ec_conf):
    """[(pulsar index, flag or None)] of a set_jitter configuration; a pulsar whose log10_ecorr is None has no group."""
    if ec_conf is None:
        return []
    out = []
    for a in range(P):
        if _pick(ec_conf["log10_ecorr"], a, P) is None:
            continue
        flags = _pick_flags(ec_conf["flags"], a, P)
        out += [(a, None)] if flags is None else [(a, f) for f in flags]
    return out


def _group_value(val, P, groups):
    """the configured value of every group of `groups` from a per-pulsar scalar / per-flag array parameter (None entries -> NaN)"""
    out = np.full(len(groups), np.nan)
    seen = {}
    for g, (a_, flag) in enumerate(groups):
        v = _pick(val, a_, P)
        ct = seen.get(a_, 0)
        seen[a_] = ct + 1
        if v is None:
            continue
        out[g] = float(v) if flag is None else float(np.asarray(v, dtype=float).ravel()[ct])
    return out


def configured_wn(P, wn_conf):
    """(efac [G_wn], equad [G_wn] in seconds, 0 = none) as prepare() computes them (10 ** log10_equad in NumPy)"""
    groups = wn_groups(P, wn_conf)
    efac = _group_value(wn_conf["efac"], P, groups)
    l10 = _group_value(wn_conf["log10_equad"], P, groups)
    with np.errstate(invalid="ignore"):
        equad = np.where(np.isnan(l10), 0.0, 10 ** l10)
    return efac, equad


def configured_ecorr(P, ec_conf):
    """ecorr [G_ec] in seconds as prepare() computes it"""
    return 10 ** _group_value(ec_conf["log10_ecorr"], P, ecorr_groups(P, ec_conf))


def psr_offsets(P, groups):
    """[P + 1] first group of every pulsar (groups are pulsar-major)"""
    n = np.bincount([a for a, _ in groups], minlength=P) if groups else np.zeros(P, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def toa_groups(groups, a, toa_flags):
    """group index of every element of toa_flags (the flag values of the TOAs, or of the epochs' first TOAs, of pulsar a), -1 where
    the flag is in no listed group; a flag listed twice belongs to the later group, as in the configured vectors"""
    out = np.full(len(toa_flags), -1, dtype=np.int32)
    for g, (a_, flag) in enumerate(groups):
        if a_ != a:
            continue
        if flag is None:
            out[:] = g
        else:
            out[np.asarray(toa_flags) == flag] = g
    return out


def check_config(keys, P, wn_conf, ec_conf, wn_mode):
    """refuse white-noise keys the configuration cannot honour (before anything is launched)"""
    keys = set(keys) & set(KEYS)
    if keys and wn_mode != "reference":
        raise ValueError(f"theta: {sorted(keys)} need wn_mode='reference' (wn_mode={wn_mode!r} draws one deviate per TOA with the configured "
                         "combined amplitude)")
    if keys & set(WN_KEYS) and wn_conf is None:
        raise ValueError(f"theta: {sorted(keys & set(WN_KEYS))} given but no white noise is configured (set_white_noise)")
    if ECORR_KEY in keys:
        if ec_conf is None:
            raise ValueError(f"theta: {ECORR_KEY} given but no ECORR is configured (set_jitter)")
        if not ecorr_groups(P, ec_conf):
            raise ValueError(f"theta: {ECORR_KEY} given but no pulsar has an ECORR (every log10_ecorr is None)")
    for kind, groups in (("white-noise", wn_groups(P, wn_conf) if keys & set(WN_KEYS) else []),
                         ("ECORR", ecorr_groups(P, ec_conf) if ECORR_KEY in keys else [])):
        per_psr = np.diff(psr_offsets(P, groups))
        if len(per_psr) and per_psr.max() > GMAX:
            raise ValueError(f"theta: pulsar {int(per_psr.argmax())} has {int(per_psr.max())} {kind} groups; per-realisation white noise "
                             f"takes at most {GMAX} per pulsar")


def check_theta(wn, R, P, wn_conf, ec_conf, wn_mode, check_values=True):
    """validate the white-noise keys of theta for R realisations; returns {key: array} (the caller's arrays, unconverted).
    check_values=False skips the value checks (labels drawn inside a validated prior)."""
    if not wn:
        return {}
    check_config(wn.keys(), P, wn_conf, ec_conf, wn_mode)
    n = {EFAC_KEY: len(wn_groups(P, wn_conf)), EQUAD_KEY: len(wn_groups(P, wn_conf)), ECORR_KEY: len(ecorr_groups(P, ec_conf))}
    out = {}
    for k, v in wn.items():
        v = _as_array(k, v)
        if tuple(v.shape) != (R, n[k]):
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {(R, n[k])}")
        if check_values and bool(_xp(v).isinf(v).any()):
            raise ValueError(f"theta[{k!r}]: infinite values (NaN alone means 'as configured')")
        out[k] = v
    return out


def refuse_td(theta):
    """TD mode: the dense factors are built for one covariance"""
    bad = sorted(k for k in theta if k in KEYS)
    if bad:
        raise ValueError(f"per-realisation theta is not supported in TD mode: {bad} would change the covariance the dense factors are built "
                         "for (only cw_* and bwm_* keys are accepted): use generate(theta=...) or generate_sampled()")


def refuse_noise_model(theta):
    """theta as the noise model of a statistic (optimal_statistic(theta=), matched=True, likelihood grids): the matched statistics hold
    white noise fixed by construction"""
    bad = sorted(k for k in theta if k in KEYS) if isinstance(theta, dict) else []
    if bad:
        raise ValueError(f"theta: {bad} cannot be part of a statistic's noise model: the matched statistics and likelihoods hold the white "
                         "noise fixed (their per-TOA weights are built once, from the configured EFAC / EQUAD / ECORR); generate under these "
                         "keys and evaluate the fixed-noise statistic, or drop them from the noise model's theta")


def make_prior(G_wn, G_ec, **boxes):
    """validated {key: (lo [n], hi [n])} of the wn_* boxes of set_hyper_prior: (lo, hi) for every group or [n, 2], n = G_wn (wn_efac,
    wn_log10_equad) or G_ec (wn_log10_ecorr); {} when none is given"""
    prior = {}
    for k, box in boxes.items():
        if box is None:
            continue
        if k not in KEYS:
            raise ValueError(f"set_hyper_prior: unknown parameter {k!r} (expected one of {list(KEYS)})")
        n = G_ec if k == ECORR_KEY else G_wn
        if n == 0:
            raise ValueError(f"set_hyper_prior: {k} needs {'set_jitter' if k == ECORR_KEY else 'set_white_noise'} (it has no group to sample)")
        b = np.asarray(box, dtype=np.float64)
        if b.shape == (2,):
            b = np.broadcast_to(b, (n, 2))
        if b.shape != (n, 2):
            raise ValueError(f"set_hyper_prior: {k} must be (lo, hi) or [{n}, 2], got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or np.any(b[:, 1] < b[:, 0]):
            raise ValueError(f"set_hyper_prior: {k} needs finite bounds with lo <= hi")
        prior[k] = (b[:, 0].copy(), b[:, 1].copy())
    return prior
