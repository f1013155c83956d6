"""Sine-Gaussian wavelets per realisation (ReplicaEngine.set_burst, set_transients): host-side validation, the column layout of the
labels, the priors and a NumPy evaluation of the terms.  Plain functions of the configuration and the arrays, so that they run (and
are tested) without a GPU, like _bwm.py.

A wavelet is g(t) cos(2 pi f (t - t0) + phi), g = exp(-1/2 ((t - t0) / tau)^2), t = mjd * 86400, t0 = t0_mjd * 86400: tau is the standard
deviation of the Gaussian envelope (the convention of the reference's golden burst).  The family stands in for the callables of the
reference's add_burst / add_noise_transient (deterministic.py:718-819).

theta may hold, next to every other key,
    burst_cos_gwtheta, burst_gwphi, burst_psi                                                              [R]
    burst_t0_mjd, burst_log10_tau [s], burst_log10_f [Hz], burst_log10_a_plus [s], burst_phase_plus,
    burst_log10_a_cross [s], burst_phase_cross                                                             [R, W]
    burst_count (optional, integer 0 .. W; wavelets at or past it are never read)                          [R]
for the GW burst h+ = sum_w A+_w g_w cos(w_w dt_w + phi+_w), hx likewise, res_a = -F+_a (h+ c2psi - hx s2psi) - Fx_a (h+ s2psi + hx c2psi),
and
    nt_psr (integer 0 .. P-1), nt_t0_mjd, nt_log10_tau, nt_log10_f, nt_log10_a [s], nt_phase               [R, V]
    nt_count (optional)                                                                                    [R]
for the noise transients res_a += sum_{v: psr_v = a} A_v g_v cos(w_v dt_v + phi_v).  All keys of a set but its count go together.

Out of scope: arbitrary callables, the pulsar term, remove_quad for transients, chromatic transients, more than one sky position.
"""
import numpy as np

from ._cw import _like, _live
from ._hyper import _as_array, _xp

W_MAX = 128
STREAM_BURST, STREAM_NT = 13, 14   # csrc/pta_burst.h

# label columns (pta_burst_uniform: stream (13, 0) for the sky row, (13, 1 + w) for wavelet w; pta_transient_uniform: stream (14, v))
SKY_COLUMNS = ("cos_gwtheta", "gwphi", "psi")
WAV_COLUMNS = ("t0_mjd", "log10_tau", "log10_f", "log10_a_plus", "phase_plus", "log10_a_cross", "phase_cross")
SKY_KEYS = tuple("burst_" + c for c in SKY_COLUMNS)
WAV_KEYS = tuple("burst_" + c for c in WAV_COLUMNS)
COUNT_KEY = "burst_count"
KEYS = SKY_KEYS + WAV_KEYS
NT_COLUMNS = ("psr", "t0_mjd", "log10_tau", "log10_f", "log10_a", "phase")
NT_KEYS = tuple("nt_" + c for c in NT_COLUMNS)
NT_COUNT_KEY = "nt_count"
PRIOR_DEFAULTS = {"cos_gwtheta": (-1.0, 1.0), "gwphi": (0.0, 2 * np.pi), "psi": (0.0, np.pi), "phase_plus": (0.0, 2 * np.pi),
                  "phase_cross": (0.0, 2 * np.pi), "phase": (0.0, 2 * np.pi)}
PRIOR_REQUIRED = ("t0_mjd", "log10_tau", "log10_f", "log10_a_plus", "log10_a_cross")
NT_PRIOR_REQUIRED = ("t0_mjd", "log10_tau", "log10_f", "log10_a")


def _n(what, name, n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= W_MAX:
        raise ValueError(f"{what}: {name} must be an integer in 1 .. {W_MAX}, got {n!r}")
    return int(n)


def make_config(n_wavelets, remove_quad=False):
    """validated set_burst() configuration"""
    return {"W": _n("set_burst", "n_wavelets", n_wavelets), "remove_quad": bool(remove_quad)}


def make_nt_config(n):
    """validated set_transients() configuration"""
    return {"V": _n("set_transients", "n", n)}


def split(theta):
    """(rest, burst, nt): the burst_* and nt_* keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    bk, nk = KEYS + (COUNT_KEY,), NT_KEYS + (NT_COUNT_KEY,)
    burst = {k: v for k, v in theta.items() if k in bk}
    nt = {k: v for k, v in theta.items() if k in nk}
    rest = {k: v for k, v in theta.items() if k not in bk and k not in nk}
    return rest, burst, nt


def has_keys(det):
    """True if a dict of validated deterministic keys holds a wavelet burst."""
    return bool(det) and KEYS[0] in det


def has_nt_keys(det):
    """True if a dict of validated deterministic keys holds noise transients."""
    return bool(det) and NT_KEYS[0] in det


def _check_count(key, count, R, n):
    c = count if isinstance(count, np.ndarray) or hasattr(count, "device") else np.asarray(count)
    if _xp(c) is np:
        integer = c.dtype.kind in "iu"
    else:
        integer = not (c.dtype.is_floating_point or c.dtype.is_complex) and str(c.dtype) != "torch.bool"
    if not integer:
        raise ValueError(f"theta[{key!r}]: expected an integer array, got dtype {c.dtype}")
    if tuple(c.shape) != (R,):
        raise ValueError(f"theta[{key!r}]: shape {tuple(c.shape)}, expected {(R,)}")
    if bool((c < 0).any()) or bool((c > n).any()):
        raise ValueError(f"theta[{key!r}]: counts must lie in 0 .. {n}")
    return c


def _check_set(keys, shapes, part, count_key, R, n, check_values, what):
    """the shared half of check_theta / check_nt_theta: all keys present, shapes, count, finite values below the count"""
    missing = [k for k in keys if k not in part]
    if missing:
        raise ValueError(f"theta: {what} keys need all of {list(keys)}; missing {missing}")
    out = {k: _as_array(k, part[k]) for k in keys}
    for k, v in out.items():
        if tuple(v.shape) != shapes[k]:
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {shapes[k]}")
    live = None
    if count_key in part:
        out[count_key] = _check_count(count_key, part[count_key], R, n)
        live = _live(out[count_key], n)
    if check_values:
        for k in keys:
            v = out[k]
            bad = ~_xp(v).isfinite(v)
            if live is not None and len(shapes[k]) == 2:
                bad = bad & _like(live, v)
            if bool(bad.any()):
                raise ValueError(f"theta[{k!r}]: non-finite values")
    return out, live


def check_theta(burst, R, conf, check_values=True):
    """validate the burst keys of theta for R realisations against make_config(); returns {key: array} (the caller's arrays,
    unconverted).  check_values=False skips the value checks (labels drawn by pta_burst_uniform inside a validated prior)."""
    if not burst:
        return {}
    if conf is None:
        raise ValueError("theta: no per-realisation wavelet burst configured (set_burst)")
    W = conf["W"]
    shapes = {k: (R,) for k in SKY_KEYS}
    shapes.update({k: (R, W) for k in WAV_KEYS})
    out, _ = _check_set(KEYS, shapes, burst, COUNT_KEY, R, W, check_values, "burst")
    if check_values and bool((abs(out["burst_cos_gwtheta"]) > 1).any()):
        raise ValueError("theta['burst_cos_gwtheta']: |cos| > 1")
    return out


def check_nt_theta(nt, R, P, conf, check_values=True):
    """validate the noise-transient keys of theta for R realisations of a P-pulsar array against make_nt_config()"""
    if not nt:
        return {}
    if conf is None:
        raise ValueError("theta: no per-realisation noise transients configured (set_transients)")
    V = conf["V"]
    out, live = _check_set(NT_KEYS, {k: (R, V) for k in NT_KEYS}, nt, NT_COUNT_KEY, R, V, check_values, "noise-transient")
    if check_values:
        p = out["nt_psr"]
        bad = (p < 0) | (p > P - 1) | (p != _xp(p).floor(p) if _is_float(p) else p != p)
        if live is not None:
            bad = bad & _like(live, p)
        if bool(bad.any()):
            raise ValueError(f"theta['nt_psr']: pulsar indices must be integers in 0 .. P-1 = {P - 1}")
    return out


def _is_float(x):
    return x.dtype.kind == "f" if _xp(x) is np else x.dtype.is_floating_point


def _boxes(what, columns, required, boxes):
    unknown = set(boxes) - set(columns)
    if unknown:
        raise ValueError(f"{what}: unknown parameter(s) {sorted(unknown)} (expected some of {list(columns)})")
    for k in required:
        if boxes.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    prior = {}
    for k in columns:
        box = boxes.get(k)
        if box is None:
            box = PRIOR_DEFAULTS[k]
        b = np.asarray(box, dtype=np.float64)
        if b.shape != (2,):
            raise ValueError(f"{what}: {k} must be (lo, hi), got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or b[1] < b[0]:
            raise ValueError(f"{what}: {k} needs finite bounds with lo <= hi")
        if k.startswith("cos_") and np.any(np.abs(b) > 1):
            raise ValueError(f"{what}: {k} must lie inside [-1, 1]")
        prior[k] = (float(b[0]), float(b[1]))
    return prior


def make_prior(**boxes):
    """validated set_burst_prior() boxes: {column name: (lo, hi)} over SKY_COLUMNS + WAV_COLUMNS.  t0_mjd, log10_tau, log10_f and the
    two amplitudes are required; the angles and phases default to their isotropic / full ranges."""
    return _boxes("set_burst_prior", SKY_COLUMNS + WAV_COLUMNS, PRIOR_REQUIRED, boxes)


def make_nt_prior(**boxes):
    """validated set_transient_prior() boxes over NT_COLUMNS without psr (drawn as the floor of U(0, P)); phase defaults to (0, 2 pi)"""
    return _boxes("set_transient_prior", NT_COLUMNS[1:], NT_PRIOR_REQUIRED, boxes)


def prior_bounds(prior):
    """lo, hi [10] of pta_burst_uniform for a make_prior() dict: the sky columns, then the wavelet columns"""
    cols = SKY_COLUMNS + WAV_COLUMNS
    return np.array([prior[c][0] for c in cols]), np.array([prior[c][1] for c in cols])


def nt_prior_bounds(prior, P):
    """lo, hi [6] of pta_transient_uniform: column 0 the box (0, P) whose floor is the pulsar"""
    return (np.array([0.0] + [prior[c][0] for c in NT_COLUMNS[1:]]), np.array([float(P)] + [prior[c][1] for c in NT_COLUMNS[1:]]))


def labels(sky, wav):
    """{theta key: column} of the sampled sky [R, 3] and wavelet [R, W, 7] tables"""
    out = {"burst_" + c: sky[:, j].contiguous() for j, c in enumerate(SKY_COLUMNS)}
    out.update({"burst_" + c: wav[:, :, j].contiguous() for j, c in enumerate(WAV_COLUMNS)})
    return out


def nt_labels(table):
    """{theta key: column} of the sampled transient table [R, V, 6]; nt_psr as int32"""
    import torch
    out = {"nt_" + c: table[:, :, j].contiguous() for j, c in enumerate(NT_COLUMNS)}
    out["nt_psr"] = out["nt_psr"].to(torch.int32)
    return out


# ---------------------------------------------------------------- NumPy evaluation (the list API's callables, tests) -----------------
def wavelet(t, t0_s, tau, f, amp=1.0, phase=0.0):
    """amp g(t) cos(2 pi f (t - t0) + phase) at t [s], in the precision of t"""
    dt = t - t0_s
    return amp * np.exp(-0.5 * (dt / tau) ** 2) * np.cos(2 * np.pi * f * dt + phase)


def waveform(wavelets, amp="log10_a", phase="phase"):
    """the callable t [s] -> sum of the wavelets (dicts with t0_mjd, log10_tau, log10_f and the named amplitude / phase columns): what
    add_wavelet_burst / add_wavelet_transient hand to the reference's add_burst / add_noise_transient"""
    rows = [(float(w["t0_mjd"]) * 86400.0, 10.0 ** float(w["log10_tau"]), 10.0 ** float(w["log10_f"]), 10.0 ** float(w[amp]), float(w[phase]))
            for w in wavelets]

    def h(t):
        out = np.zeros(np.shape(t), dtype=np.result_type(np.asarray(t).dtype, np.float64))
        for t0, tau, f, a, ph in rows:
            out = out + wavelet(t, t0, tau, f, a, ph)
        return out
    return h


def quad_basis(toa_s_list):
    """[n_toa, 3]: per pulsar an orthonormal basis Q_a of (1, t, t^2) over its TOAs (centred and scaled in long double, then QR), so
    that term - Q_a (Q_a^T term) is the residual of the reference's unweighted degree-2 polyfit; zero rows for a pulsar of <= 3 TOAs,
    whose term is zero"""
    out = []
    for t in toa_s_list:
        t = np.asarray(t, dtype=np.longdouble)
        n = len(t)
        if n <= 3:
            out.append(np.zeros((n, 3)))
            continue
        mid, half = (t.max() + t.min()) / 2, max((t.max() - t.min()) / 2, np.longdouble(1))
        x = np.asarray((t - mid) / half, dtype=np.float64)
        q, _ = np.linalg.qr(np.stack([np.ones(n), x, x * x], axis=1))
        out.append(q)
    return np.ascontiguousarray(np.concatenate(out, axis=0))


def burst_term(toa_s, fplus, fcross, psi, wavelets, dtype=np.float64):
    """the burst of one pulsar in NumPy at precision dtype: -F+ (h+ c2 - hx s2) - Fx (h+ s2 + hx c2), wavelets = dicts of WAV_COLUMNS"""
    t = np.asarray(toa_s, dtype=dtype)
    hp, hc = waveform(wavelets, "log10_a_plus", "phase_plus")(t), waveform(wavelets, "log10_a_cross", "phase_cross")(t)
    c2, s2 = np.cos(2 * dtype(psi)), np.sin(2 * dtype(psi))
    return -dtype(fplus) * (hp * c2 - hc * s2) - dtype(fcross) * (hp * s2 + hc * c2)
