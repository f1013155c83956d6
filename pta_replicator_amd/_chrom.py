"""One chromatic Gaussian process per pulsar (DM variations at index 2): the row weights, the configuration of
ReplicaEngine.set_chromatic_noise, theta's chrom_* keys, their prior boxes and the refusals.  Plain functions of the configuration and
the arrays, so that they run (and are tested) without a GPU, like _cw.py, _bwm.py and _wn_hyper.py.

    dt_i = (nu_ref / nu_i)^chi sum_k F_ik y_k,   y_k = sqrt(phi_k) z_k

F and phi are the red noise's (red_noise.py:106-128: sin / cos columns at k / Tspan, phi = A^2 (f / f_yr)^-gamma / (12 pi^2 Tspan) yr^3);
z is deviate k of stream (STREAM_CHROM, pulsar).  theta may hold, next to the keys of _hyper, _cw, _bwm and _wn_hyper,
    chrom_log10_A, chrom_gamma   [R, P]
with the rules of rn_log10_A / rn_gamma: a key that is not given keeps its configured value, NaN in chrom_log10_A means "this pulsar as
configured", a pulsar configured without the process keeps none whatever its entries say.

Out of scope: TD mode, the theta-matched statistics and likelihoods, a second process, chi per realisation.
"""
import numpy as np

from ._hyper import _as_array, _host, _xp
from .constants import YEAR_IN_SEC

STREAM_CHROM = 10   # PTA_STREAM_CHROM (csrc/pta_rng.h): stream_id(10, pulsar), pair c >> 1, branch c & 1 = coefficient c
A_KEY, GAMMA_KEY = "chrom_log10_A", "chrom_gamma"
KEYS = (A_KEY, GAMMA_KEY)
# prior draws: pta_hyper_uniform_field on stream (7, FIELD[key]), pair = pulsar (fields 0 .. 5: _hyper, _wn_hyper.FIELD)
FIELD = {A_KEY: 6, GAMMA_KEY: 7}


def weights(freqs_mhz, index=2.0, ref_freq_mhz=1400.0, name="the pulsar"):
    """w_i = (nu_ref / nu_i)^chi [N], NumPy's ** on float64; a non-finite or non-positive frequency is refused by name"""
    nu = np.asarray(freqs_mhz, dtype=np.float64)
    bad = ~np.isfinite(nu) | (nu <= 0)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"chromatic noise: {name} has a non-finite or non-positive radio frequency (TOA {i}: {float(nu.ravel()[i])} MHz)")
    return (float(ref_freq_mhz) / nu) ** float(index)


def toa_freqs(psr):
    """radio frequencies [MHz] of a pulsar's TOAs from wherever the object holds them: toas.freqs_mhz first, then toas.get_freqs()
    (the order of ReplicaEngine.to_enterprise)"""
    toas = psr.toas
    freq = getattr(toas, "freqs_mhz", None)
    if freq is None:
        try:
            freq = np.asarray(toas.get_freqs().to("MHz").value, dtype=np.float64)
        except AttributeError:
            raise ValueError(f"chromatic noise: pulsar {getattr(psr, 'name', '?')} holds no radio frequencies (toas.freqs_mhz or "
                             "toas.get_freqs())") from None
    n = len(toas.get_mjds().value)
    return np.asarray(freq, dtype=np.float64) * np.ones(n)


def check_scalars(index, ref_freq_mhz, components, who):
    if isinstance(components, bool) or not isinstance(components, (int, np.integer)) or int(components) < 1:
        raise ValueError(f"{who}: components={components!r} must be an integer >= 1")
    if not np.isfinite(float(index)):
        raise ValueError(f"{who}: index={index!r} must be finite")
    if not (np.isfinite(float(ref_freq_mhz)) and float(ref_freq_mhz) > 0):
        raise ValueError(f"{who}: ref_freq_mhz={ref_freq_mhz!r} must be finite and positive")


def make_config(P, log10_amplitude, spectral_index, components=30, index=2.0, ref_freq_mhz=1400.0):
    """validated set_chromatic_noise() configuration: amplitude and spectral index per pulsar (a scalar or a list, None = no process
    for that pulsar), as set_red_noise takes them"""
    check_scalars(index, ref_freq_mhz, components, "set_chromatic_noise")
    try:
        A = list(np.broadcast_to(np.asarray(log10_amplitude, dtype=object), (P,)))
        g = list(np.broadcast_to(np.asarray(spectral_index, dtype=object), (P,)))
    except ValueError:
        raise ValueError(f"set_chromatic_noise: log10_amplitude / spectral_index must be scalars or one entry per pulsar ({P})") from None
    return dict(A=A, g=g, components=int(components), index=float(index), ref=float(ref_freq_mhz))


def configured(conf):
    """configured (log10_A, gamma) [P] of every pulsar, NaN where it has no process"""
    none = [a is None or g is None for a, g in zip(conf["A"], conf["g"])]
    lA = np.array([np.nan if n else float(a) for n, a in zip(none, conf["A"])])
    g = np.array([np.nan if n else float(g_) for n, g_ in zip(none, conf["g"])])
    return lA, g


def prior_phi(f, Tspan, log10_A, gamma):
    """phi [2 len(f)] of the sin / cos columns at frequencies f: the reference's expression (red_noise.py:112-126)"""
    freqs = np.repeat(f, 2)
    fyr = 1 / YEAR_IN_SEC
    return (10 ** log10_A) ** 2 * (freqs / fyr) ** (-gamma) / (12 * np.pi ** 2 * Tspan) * YEAR_IN_SEC ** 3


def split(theta):
    """(rest, chrom): the chromatic keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    ch = {k: v for k, v in theta.items() if k in KEYS}
    rest = {k: v for k, v in theta.items() if k not in KEYS}
    return rest, ch


def has_keys(det):
    """True if a dict of validated keys (the second member of ReplicaEngine._theta_parts) holds chromatic keys."""
    return bool(det) and any(k in det for k in KEYS)


def check_theta(keys, R, P, conf, check_values=True):
    """validate theta's chromatic keys for R realisations of a P-pulsar array against the configuration (None: no process); returns
    {key: array} (the caller's arrays, unconverted), {} without keys.  The rules of rn_log10_A / rn_gamma (_hyper._check_arrays)."""
    if not keys:
        return {}
    if conf is None:
        raise ValueError(f"theta: chromatic-noise parameters {sorted(keys)} given but no chromatic process is configured (set_chromatic_noise)")
    out = {}
    for k, v in keys.items():
        v = _as_array(k, v)
        if tuple(v.shape) != (R, P):
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {(R, P)}")
        out[k] = v
    if not check_values:
        return out
    if A_KEY in out:
        a = out[A_KEY]
        if bool(_xp(a).isinf(a).any()):
            raise ValueError(f"theta[{A_KEY!r}]: infinite values (NaN alone means 'as configured')")
    if GAMMA_KEY in out:
        g = _host(out[GAMMA_KEY])
        if A_KEY in out:
            sampled = ~np.isnan(_host(out[A_KEY]))
        else:   # index given, amplitude as configured: every pulsar that has the process needs a finite index
            sampled = np.broadcast_to(~np.isnan(configured(conf)[0]), (R, P))
        if bool((np.isinf(g) | (np.isnan(g) & sampled)).any()):
            raise ValueError(f"theta[{GAMMA_KEY!r}]: non-finite values where the amplitude is sampled")
    return out


def make_prior(P, **boxes):
    """validated {key: (lo [P], hi [P])} of the chrom_* boxes of set_hyper_prior: (lo, hi) for every pulsar or [P, 2]; {} when none is
    given"""
    prior = {}
    for k, box in boxes.items():
        if box is None:
            continue
        if k not in KEYS:
            raise ValueError(f"set_hyper_prior: unknown parameter {k!r} (expected one of {list(KEYS)})")
        b = np.asarray(box, dtype=np.float64)
        if b.shape == (2,):
            b = np.broadcast_to(b, (P, 2))
        if b.shape != (P, 2):
            raise ValueError(f"set_hyper_prior: {k} must be (lo, hi) or [{P}, 2], got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or np.any(b[:, 1] < b[:, 0]):
            raise ValueError(f"set_hyper_prior: {k} needs finite bounds with lo <= hi")
        prior[k] = (b[:, 0].copy(), b[:, 1].copy())
    return prior


def refuse_td(conf, who="TD mode"):
    """TD mode: the dense factors would need the chromatic term in the covariance"""
    if conf is not None:
        raise ValueError(f"{who}: an engine with a chromatic process (set_chromatic_noise) has no TD mode - the dense factors are built "
                         "from white noise, ECORR and red noise, and the chromatic term is not in that covariance: use generate()")


def refuse_noise_model(theta):
    """theta as the noise model of a statistic (optimal_statistic(theta=), matched=True, likelihood grids)"""
    bad = sorted(k for k in theta if k in KEYS) if isinstance(theta, dict) else []
    if bad:
        raise ValueError(f"theta: {bad} cannot be part of a statistic's noise model: the matched statistics and likelihoods carry no "
                         "chromatic term; generate under these keys and evaluate the fixed-noise statistic")


def refuse_matched(conf, who):
    """the theta-matched OS and the likelihood: their fixed part is white noise + ECORR only"""
    if conf is not None:
        raise ValueError(f"{who}: not available on an engine with a chromatic process (set_chromatic_noise) - the fixed part of this noise "
                         "model is white noise + ECORR only, and a fixed low-rank chromatic term is not part of it; the fixed-noise "
                         "statistics (prepare_optimal_statistic(), prepare_f_statistic, prepare_bwm_statistic) carry it")
