"""One burst with memory per realisation (ReplicaEngine.set_bwm): host-side validation and the column layout of the burst labels.
Plain functions of the configuration and the arrays, so that they run (and are tested) without a GPU, like _cw.py.

theta may hold, next to the GWB / red-noise keys of _hyper and the cw_* keys of _cw,
    bwm_log10_h (strain), bwm_cos_gwtheta, bwm_gwphi, bwm_psi (the reference's bwm_pol), bwm_t0_mjd     [R]
as NumPy arrays or torch tensors.  If any of them is given, all five must be.  The signal is the reference's add_gw_memory
(deterministic.py:822-884): 0 before the epoch, h (cos 2psi F+ + sin 2psi Fx) (t - t0) from it on, t = mjd * 86400.

Out of scope: the pulsar term, more than one burst per realisation.
"""
import numpy as np

from ._hyper import _as_array, _xp

# label columns of the burst table (pta_bwm_uniform: stream kind 9, pair = column)
COLUMNS = ("cos_gwtheta", "gwphi", "log10_h", "psi", "t0_mjd")
KEYS = tuple("bwm_" + c for c in COLUMNS)
N_SRC = len(COLUMNS)
PRIOR_DEFAULTS = {"cos_gwtheta": (-1.0, 1.0), "gwphi": (0.0, 2 * np.pi), "psi": (0.0, np.pi)}
PRIOR_REQUIRED = ("log10_h", "t0_mjd")


def split(theta):
    """(rest, bwm): the BWM keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    bwm = {k: v for k, v in theta.items() if k in KEYS}
    rest = {k: v for k, v in theta.items() if k not in KEYS}
    return rest, bwm


def has_keys(det):
    """True if a dict of validated deterministic keys (cw_* and bwm_*) holds a burst."""
    return bool(det) and KEYS[0] in det


def check_theta(bwm, R, configured, check_values=True):
    """validate the BWM keys of theta for R realisations; returns {key: array} (the caller's arrays, unconverted).
    check_values=False skips the value checks (labels drawn by pta_bwm_uniform inside a validated prior)."""
    if not bwm:
        return {}
    if not configured:
        raise ValueError("theta: no per-realisation burst with memory configured (set_bwm)")
    missing = [k for k in KEYS if k not in bwm]
    if missing:
        raise ValueError(f"theta: BWM keys need all of {list(KEYS)}; missing {missing}")
    out = {k: _as_array(k, bwm[k]) for k in KEYS}
    for k, v in out.items():
        if tuple(v.shape) != (R,):
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {(R,)}")
    if not check_values:
        return out
    for k, v in out.items():
        if bool((~_xp(v).isfinite(v)).any()):
            raise ValueError(f"theta[{k!r}]: non-finite values")
    if bool((abs(out["bwm_cos_gwtheta"]) > 1).any()):
        raise ValueError("theta['bwm_cos_gwtheta']: |cos| > 1")
    return out


def make_prior(**boxes):
    """validated set_bwm_prior() boxes: {column name: (lo, hi)}.  log10_h and t0_mjd are required; the angles default to the
    isotropic boxes."""
    unknown = set(boxes) - set(COLUMNS)
    if unknown:
        raise ValueError(f"set_bwm_prior: unknown parameter(s) {sorted(unknown)} (expected some of {list(COLUMNS)})")
    for k in PRIOR_REQUIRED:
        if boxes.get(k) is None:
            raise ValueError(f"set_bwm_prior: {k} is required")
    prior = {}
    for k in COLUMNS:
        box = boxes.get(k)
        if box is None:
            box = PRIOR_DEFAULTS[k]
        b = np.asarray(box, dtype=np.float64)
        if b.shape != (2,):
            raise ValueError(f"set_bwm_prior: {k} must be (lo, hi), got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or b[1] < b[0]:
            raise ValueError(f"set_bwm_prior: {k} needs finite bounds with lo <= hi")
        if k.startswith("cos_") and np.any(np.abs(b) > 1):
            raise ValueError(f"set_bwm_prior: {k} must lie inside [-1, 1]")
        prior[k] = (float(b[0]), float(b[1]))
    return prior


def prior_bounds(prior):
    """lo, hi [N_SRC] of pta_bwm_uniform for a make_prior() dict."""
    return np.array([prior[c][0] for c in COLUMNS]), np.array([prior[c][1] for c in COLUMNS])


def labels(table):
    """{theta key: column of the [R, N_SRC] table} of sampled labels."""
    return {"bwm_" + c: table[:, j].contiguous() for j, c in enumerate(COLUMNS)}


def ramp(coef, t0_s, toa_s):
    """the term in NumPy from the device's tables: coef [...], t0_s [...] broadcast against toa_s (tests)."""
    coef, t0_s, toa_s = (np.asarray(x, dtype=np.float64) for x in (coef, t0_s, toa_s))
    return np.where(toa_s < t0_s, 0.0, coef * (toa_s - t0_s))
