"""Common red processes with an ORF of their own (ReplicaEngine.add_common_process: a clock error = monopole, an ephemeris error =
dipole, CURN, HD, or a [P, P] array): the configuration, the host tables, theta's cp_* keys, their prior boxes and the refusals.  Plain
functions of the configuration and the arrays, so that they run (and are tested) without a GPU, like _chrom.py.

Process p of up to MAX adds, on the array-wide Fourier basis the likelihoods and the OS model a common process on (times mjd * 86400,
T = the span of the whole array, f_k = k / T, sin column then cos column: optimal_statistic.fourier_basis),

    dt_{a,i} += sum_c F_ic y_ac,   y_ac = sqrt(phi_pc(log10_A, gamma)) sum_j B_p[a, j] z_pcj

phi the red-noise prior with Tspan = T, B_p = orf_factor(orf_matrix(orf, pos)) [P, rho_p], z deviate n = c rho_p + j of stream
(STREAM_CPROC, p): pair n >> 1, branch n & 1.  theta may hold, next to every other key,
    cp_log10_A, cp_gamma   [R, n_proc]
with the rules of the chromatic keys: a key that is not given keeps its configured value, NaN in cp_log10_A means "this process as
configured".

Out of scope: TD mode, the theta-matched statistics and likelihoods, the cross-correlations of the process inside C of the OS, a
spectrum other than a power law, more than four processes, an ORF that depends on theta.
"""
import numpy as np

from . import optimal_statistic as ost
from ._hyper import _as_array, _host, _xp
from .constants import YEAR_IN_SEC

STREAM_CPROC = 12   # PTA_STREAM_CPROC (csrc/pta_cproc.h): stream_id(12, process), deviate n = c rho + j: pair n >> 1, branch n & 1
MAX = 4             # PTA_CPROC_MAX
A_KEY, GAMMA_KEY = "cp_log10_A", "cp_gamma"
KEYS = (A_KEY, GAMMA_KEY)
# prior draws: pta_hyper_uniform_field on stream (7, FIELD[key]), pair = process (fields 0 .. 7: _hyper, _wn_hyper.FIELD, _chrom.FIELD)
FIELD = {A_KEY: 8, GAMMA_KEY: 9}


def make_process(pos, log10_amplitude, spectral_index, orf="curn", components=14, who="add_common_process"):
    """one validated process: {A, g, components, orf (its name, or "array"), Gamma [P, P], B [P, rho]}.  pos [P, 3]: unit vectors.
    orf_matrix / orf_factor refuse an unknown name, an array that is not finite, symmetric and [P, P], one that is not positive
    semi-definite and rank 0."""
    if isinstance(components, bool) or not isinstance(components, (int, np.integer)) or not 1 <= int(components) <= 32:
        raise ValueError(f"{who}: components={components!r}: an integer 1 .. 32 (2 n_f <= 64 columns)")
    try:
        lA, g = float(log10_amplitude), float(spectral_index)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: log10_amplitude and spectral_index must be scalars (one process per call)") from None
    if not (np.isfinite(lA) and np.isfinite(g)):
        raise ValueError(f"{who}: log10_amplitude={log10_amplitude!r} and spectral_index={spectral_index!r} must be finite")
    Gamma = ost.orf_matrix(orf, pos)
    B = np.ascontiguousarray(ost.orf_factor(Gamma))
    return dict(A=lA, g=g, components=int(components), orf=orf if isinstance(orf, str) else "array", Gamma=Gamma, B=B)


def add(procs, proc, who="add_common_process"):
    """the list with one more process; a fifth is refused"""
    procs = list(procs or [])
    if len(procs) >= MAX:
        raise ValueError(f"{who}: at most {MAX} common processes per engine")
    return procs + [proc]


def configured(procs):
    """configured (log10_A, gamma) [n_proc]"""
    return np.array([p["A"] for p in procs]), np.array([p["g"] for p in procs])


def prior_phi(nf, T, log10_A, gamma):
    """phi [2 nf] of the sin / cos columns at f_k = k / T: the red-noise prior with Tspan = T (_chrom.prior_phi)"""
    freqs = np.repeat(np.arange(1, nf + 1) / float(T), 2)
    fyr = 1 / YEAR_IN_SEC
    return (10 ** log10_A) ** 2 * (freqs / fyr) ** (-gamma) / (12 * np.pi ** 2 * T) * YEAR_IN_SEC ** 3


def span(toas_s):
    """T of the array: the span of all TOAs [s], as optimal_statistic.array_basis forms it"""
    return max(float(np.max(t)) for t in toas_s) - min(float(np.min(t)) for t in toas_s)


def sincos1(toas_s, T):
    """[N, 2] float64 (sin, cos)(2 pi x), x = frac(t / T), the quotient, its fraction and the functions in long double: what the add
    kernel builds every harmonic from"""
    t = np.asarray(toas_s, dtype=np.float64).astype(np.longdouble)
    x = t / np.longdouble(T)
    x = x - np.floor(x)
    arg = (np.longdouble(2) * _pi_ld()) * x
    return np.stack([np.sin(arg), np.cos(arg)], axis=1).astype(np.float64)


def _pi_ld():
    """pi to long-double precision (numpy.pi is the float64 value)"""
    return np.longdouble(4) * np.arctan(np.longdouble(1))


def host_tables(procs, toas_s):
    """the host half of the tables, NumPy alone: T, K = 2 x the most components, kp / rho [n_proc], amp [n_proc, K] the configured
    sqrt(phi) (zero beyond a process's columns), sc1 [n_toa, 2] over the concatenated TOAs, B the factors"""
    T = span(toas_s)
    if not T > 0:
        raise ValueError("add_common_process: the array's TOAs span no time (T = 0): the basis k / T does not exist")
    K = 2 * max(p["components"] for p in procs)
    amp = np.zeros((len(procs), K))
    for i, p in enumerate(procs):
        amp[i, :2 * p["components"]] = np.sqrt(prior_phi(p["components"], T, p["A"], p["g"]))
    return dict(T=T, K=K, kp=[2 * p["components"] for p in procs], rho=[p["B"].shape[1] for p in procs], amp_host=amp,
                sc1_host=np.concatenate([sincos1(t, T) for t in toas_s]), B_host=[p["B"] for p in procs])


def low_rank_host(procs, toas_s, T=None):
    """(F [P][N_a, 2 nf_max], phi [P][2 nf_max]): the auto-term of every process, the columns F with sum_p Gamma_p,aa phi_p - what
    the fixed-noise statistics add to the low-rank part of C_a (the processes share the basis, so their variances add per column)"""
    T = span(toas_s) if T is None else T
    nf = max(p["components"] for p in procs)
    F, phi = [], []
    for a, t in enumerate(toas_s):
        F.append(ost.fourier_basis(t, nf, T))
        v = np.zeros(2 * nf)
        for p in procs:
            v[:2 * p["components"]] += p["Gamma"][a, a] * prior_phi(p["components"], T, p["A"], p["g"])
        phi.append(v)
    return F, phi


def split(theta):
    """(rest, cp): the common-process keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    cp = {k: v for k, v in theta.items() if k in KEYS}
    rest = {k: v for k, v in theta.items() if k not in KEYS}
    return rest, cp


def has_keys(det):
    """True if a dict of validated keys (the second member of ReplicaEngine._theta_parts) holds common-process keys."""
    return bool(det) and any(k in det for k in KEYS)


def check_theta(keys, R, procs, check_values=True):
    """validate theta's cp_* keys for R realisations against the configured processes (None / []: none); returns {key: array} (the
    caller's arrays, unconverted), {} without keys.  The rules of chrom_log10_A / chrom_gamma (_chrom.check_theta)."""
    if not keys:
        return {}
    if not procs:
        raise ValueError(f"theta: common-process parameters {sorted(keys)} given but no common process is configured (add_common_process)")
    n = len(procs)
    out = {}
    for k, v in keys.items():
        v = _as_array(k, v)
        if tuple(v.shape) != (R, n):
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {(R, n)}")
        out[k] = v
    if not check_values:
        return out
    if A_KEY in out:
        a = out[A_KEY]
        if bool(_xp(a).isinf(a).any()):
            raise ValueError(f"theta[{A_KEY!r}]: infinite values (NaN alone means 'as configured')")
    if GAMMA_KEY in out:
        g = _host(out[GAMMA_KEY])
        sampled = ~np.isnan(_host(out[A_KEY])) if A_KEY in out else np.ones((R, n), dtype=bool)   # index alone: every process needs it
        if bool((np.isinf(g) | (np.isnan(g) & sampled)).any()):
            raise ValueError(f"theta[{GAMMA_KEY!r}]: non-finite values where the amplitude is sampled")
    return out


def make_prior(n_proc, **boxes):
    """validated {key: (lo [n_proc], hi [n_proc])} of the cp_* boxes of set_hyper_prior: (lo, hi) for every process or [n_proc, 2]; {}
    when none is given"""
    prior = {}
    for k, box in boxes.items():
        if box is None:
            continue
        if k not in KEYS:
            raise ValueError(f"set_hyper_prior: unknown parameter {k!r} (expected one of {list(KEYS)})")
        if not n_proc:
            raise ValueError(f"set_hyper_prior: {k} given but no common process is configured (add_common_process)")
        b = np.asarray(box, dtype=np.float64)
        if b.shape == (2,):
            b = np.broadcast_to(b, (n_proc, 2))
        if b.shape != (n_proc, 2):
            raise ValueError(f"set_hyper_prior: {k} must be (lo, hi) or [{n_proc}, 2], got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or np.any(b[:, 1] < b[:, 0]):
            raise ValueError(f"set_hyper_prior: {k} needs finite bounds with lo <= hi")
        prior[k] = (b[:, 0].copy(), b[:, 1].copy())
    return prior


def refuse_td(procs, who="TD mode"):
    """TD mode: the dense factors would need the common processes in the covariance"""
    if procs:
        raise ValueError(f"{who}: an engine with a common process (add_common_process) has no TD mode - the dense factors are built "
                         "from white noise, ECORR and red noise, and the common processes are not in that covariance: use generate()")


def refuse_noise_model(theta):
    """theta as the noise model of a statistic (optimal_statistic(theta=), matched=True, likelihood grids)"""
    bad = sorted(k for k in theta if k in KEYS) if isinstance(theta, dict) else []
    if bad:
        raise ValueError(f"theta: {bad} cannot be part of a statistic's noise model: the matched statistics and likelihoods carry no "
                         "added common process; generate under these keys and evaluate the fixed-noise statistic")


def refuse_matched(procs, who):
    """the theta-matched OS and the likelihood: their fixed part is white noise + ECORR only"""
    if procs:
        raise ValueError(f"{who}: not available on an engine with a common process (add_common_process) - the fixed part of this noise "
                         "model is white noise + ECORR only, and a fixed low-rank common-process term is not part of it; the fixed-noise "
                         "statistics (prepare_optimal_statistic(), prepare_f_statistic, prepare_bwm_statistic, "
                         "prepare_correlated_likelihood) carry it")
