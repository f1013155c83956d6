"""Chromatic events per realisation (ReplicaEngine.set_chromatic_events): host-side validation, the column layout of the labels, the
per-slot prior boxes and a NumPy evaluation of the definition.  Plain functions of the configuration and the arrays, so that they run
(and are tested) without a GPU, like _burst.py.

An event lives in one pulsar.  With t = mjd * 86400, nu_i the TOA's radio frequency [MHz], t0 = t0_mjd * 86400, A = 10^log10_a [s at
nu_ref], s = -1 if sign < 0 else +1, chi = index, tau = 10^log10_tau [s],

    dt_i = s A (nu_ref / nu_i)^chi shape(t_i)

    kind 0  decay    t >= t0: exp(-(t - t0) / tau)          t < t0: 0
    kind 1  cusp     t >= t0: exp(-(t - t0) / tau)          t < t0: exp(-(t0 - t) / tau_pre)     (tau_pre = tau if log10_tau_pre is NaN)
    kind 2  bump     exp(-1/2 ((t - t0) / tau)^2)
    kind 3  annual   sin(2 pi t / YEAR_IN_SEC + phase)      (t0, tau unused)

(csrc/pta_chrom_event.h; a TOA at exactly t0 takes the t >= t0 side).  theta may hold, next to every other key,
    ce_psr (integer 0 .. P-1), ce_kind (0 .. 3 or "decay" / "cusp" / "bump" / "annual"), ce_t0_mjd, ce_log10_tau, ce_log10_a     [R, E]
    ce_log10_tau_pre (NaN = symmetric, the default), ce_sign (-1), ce_index (2), ce_phase (0)                                  [R, E]
    ce_count (optional, integer 0 .. E; events at or past it are never read)                                                    [R]

Out of scope: the solar wind, a detection statistic or likelihood for events, events in a statistic's noise model, a periodic kind at
another frequency than 1 / yr, dump_draws / replay.
"""
import numpy as np

from ._burst import _check_count, _is_float
from ._cw import _like, _live
from ._hyper import _as_array, _xp
from .constants import YEAR_IN_SEC

E_MAX = 128
STREAM_CE = 15   # csrc/pta_chrom_event.h: stream (15, e) draws slot e, pair = label column
COLUMNS = ("psr", "kind", "t0_mjd", "log10_tau", "log10_tau_pre", "log10_a", "sign", "index", "phase")
KEYS = tuple("ce_" + c for c in COLUMNS)
COUNT_KEY = "ce_count"
REQUIRED = ("ce_psr", "ce_kind", "ce_t0_mjd", "ce_log10_tau", "ce_log10_a")
DEFAULTS = {"ce_log10_tau_pre": np.nan, "ce_sign": -1.0, "ce_index": 2.0, "ce_phase": 0.0}
KINDS = ("decay", "cusp", "bump", "annual")
TABLE = ("psr", "kind", "t0_s", "inv_tau", "inv_tau_pre", "nh", "sign", "ln_a", "chi", "turns")   # the row pta_engine_chrom_event_params writes


def make_config(n=1, ref_freq_mhz=1400.0):
    """validated set_chromatic_events() configuration"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= E_MAX:
        raise ValueError(f"set_chromatic_events: n must be an integer in 1 .. {E_MAX}, got {n!r}")
    try:
        ok = np.isfinite(float(ref_freq_mhz)) and float(ref_freq_mhz) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"set_chromatic_events: ref_freq_mhz={ref_freq_mhz!r} must be finite and positive")
    return {"E": int(n), "ref_freq_mhz": float(ref_freq_mhz)}


def log_freq_ratio(freqs_mhz, ref_freq_mhz=1400.0, name="the pulsar"):
    """lnu_i = ln(nu_ref / nu_i) [N] in long double, rounded to float64; a non-finite or non-positive frequency is refused by name
    (_chrom.weights' rule)"""
    nu = np.asarray(freqs_mhz, dtype=np.float64)
    bad = ~np.isfinite(nu) | (nu <= 0)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"chromatic events: {name} has a non-finite or non-positive radio frequency (TOA {i}: {float(nu.ravel()[i])} MHz)")
    return np.asarray(np.log(np.longdouble(ref_freq_mhz) / nu.astype(np.longdouble)), dtype=np.float64)


def split(theta):
    """(rest, ce): the ce_* keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    ce = {k: v for k, v in theta.items() if isinstance(k, str) and k.startswith("ce_")}
    return {k: v for k, v in theta.items() if k not in ce}, ce


def has_keys(det):
    """True if a dict of validated deterministic keys holds chromatic events."""
    return bool(det) and KEYS[0] in det


def kind_code(kind, what="kind"):
    """0 .. 3 of an integer or a name of KINDS"""
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"{what}: unknown kind {kind!r} (expected one of {list(KINDS)} or 0 .. 3)")
        return KINDS.index(kind)
    if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or not 0 <= int(kind) <= 3:
        raise ValueError(f"{what}: kind {kind!r} must be an integer in 0 .. 3 or one of {list(KINDS)}")
    return int(kind)


def _kinds(v):
    """ce_kind as given -> an array of numbers: names become their codes"""
    if not isinstance(v, np.ndarray) and hasattr(v, "device"):   # a tensor (NumPy arrays have .device too)
        return v
    a = np.asarray(v)
    if a.dtype.kind not in "USO":
        return v
    flat = [kind_code(k, "theta['ce_kind']") if isinstance(k, str) else k for k in a.ravel().tolist()]
    try:
        return np.array(flat, dtype=np.float64).reshape(a.shape)
    except (TypeError, ValueError):
        raise ValueError("theta['ce_kind']: expected integers 0 .. 3 or names of " + str(list(KINDS))) from None


def _integers_in(v, lo, hi):
    """mask of the entries of v that are no integer in lo .. hi"""
    bad = (v < lo) | (v > hi)
    if _is_float(v):
        bad = bad | (v != _xp(v).floor(v)) | ~_xp(v).isfinite(v)
    return bad


def check_theta(ce, R, P, conf, check_values=True):
    """validate the ce_* keys of theta for R realisations of a P-pulsar array against make_config(); returns {key: array} with every
    column present (a key not given filled with its default; the caller's arrays otherwise, unconverted).  check_values=False skips
    the value checks (labels drawn by pta_chrom_event_uniform inside a validated prior)."""
    if not ce:
        return {}
    if conf is None:
        raise ValueError(f"theta: no per-realisation chromatic events configured (set_chromatic_events); got {sorted(ce)}")
    unknown = sorted(set(ce) - set(KEYS) - {COUNT_KEY})
    if unknown:
        raise ValueError(f"theta: unknown chromatic-event key(s) {unknown} (expected some of {list(KEYS) + [COUNT_KEY]})")
    missing = [k for k in REQUIRED if k not in ce]
    if missing:
        raise ValueError(f"theta: chromatic-event keys need all of {list(REQUIRED)}; missing {missing}")
    E = conf["E"]
    out = {}
    for k in KEYS:
        if k not in ce:
            out[k] = np.full((R, E), DEFAULTS[k])
            continue
        v = out[k] = _as_array(k, _kinds(ce[k]) if k == "ce_kind" else ce[k])
        if tuple(v.shape) != (R, E):
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {(R, E)}")
    live = None
    if COUNT_KEY in ce:
        out[COUNT_KEY] = _check_count(COUNT_KEY, ce[COUNT_KEY], R, E)
        live = _live(out[COUNT_KEY], E)
    if not check_values:
        return out

    def refuse(k, bad, why):
        if live is not None:
            bad = bad & _like(live, bad)
        if bool(bad.any()):
            raise ValueError(f"theta[{k!r}]: {why}")
    refuse("ce_psr", _integers_in(out["ce_psr"], 0, P - 1), f"pulsar indices must be integers in 0 .. P-1 = {P - 1}")
    refuse("ce_kind", _integers_in(out["ce_kind"], 0, 3), f"kinds must be integers in 0 .. 3 or names of {list(KINDS)}")
    for k in KEYS[2:]:
        v = out[k]
        if not _is_float(v):
            continue
        xp = _xp(v)
        refuse(k, xp.isinf(v) if k == "ce_log10_tau_pre" else ~xp.isfinite(v), "non-finite values")
    refuse("ce_sign", out["ce_sign"] == 0, "the sign must be non-zero")
    return out


# ---------------------------------------------------------------- the prior ----------------------------------------------------------
def _per_slot(name, x, E):
    """an argument of make_prior -> E entries: a list holds one entry per slot, anything else is every slot's"""
    if isinstance(x, list):
        if len(x) != E:
            raise ValueError(f"set_chromatic_event_prior: {name} is a list of {len(x)} entries, expected one per slot, E = {E}")
        return list(x)
    return [x] * E


def _box(name, x, e, nan_ok=False):
    """a scalar or a (lo, hi) pair -> (lo, hi) floats"""
    try:
        b = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        b = None
    if b is None or b.shape not in ((), (2,)):
        raise ValueError(f"set_chromatic_event_prior: {name} of slot {e} must be a number or (lo, hi), got {x!r}")
    lo, hi = (float(b), float(b)) if b.shape == () else (float(b[0]), float(b[1]))
    if nan_ok and np.isnan(lo) and np.isnan(hi):
        return lo, hi
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo:
        raise ValueError(f"set_chromatic_event_prior: {name} of slot {e} needs finite bounds with lo <= hi, got {x!r}")
    return lo, hi


def make_prior(E, P, kind, log10_a, psr=None, t0_mjd=None, log10_tau=None, log10_tau_pre=None, sign=-1, index=2.0, phase=(0.0, 2 * np.pi)):
    """validated set_chromatic_event_prior() boxes for E slots on a P-pulsar array: {"kind": [E] int, "lo", "hi": [E, 9]}.  Every
    argument is a scalar (the column is fixed: a degenerate box), a box (lo, hi), or a list of E of those, one per slot.  kind is fixed
    per slot.  psr=None draws the pulsar from U(0, P), floored; sign="random" is the box (-1, 1); log10_tau_pre=None is the NaN label
    (symmetric).  t0_mjd and log10_tau are required for slots of kinds 0 - 2 and default to 0 for the annual kind, which ignores them."""
    if log10_a is None:
        raise ValueError("set_chromatic_event_prior: log10_a is required")
    if kind is None:
        raise ValueError("set_chromatic_event_prior: kind is required")
    kinds = [kind_code(k, "set_chromatic_event_prior") for k in _per_slot("kind", kind, E)]
    args = {"psr": psr, "t0_mjd": t0_mjd, "log10_tau": log10_tau, "log10_tau_pre": log10_tau_pre, "log10_a": log10_a, "sign": sign, "index": index,
            "phase": phase}
    slots = {k: _per_slot(k, v, E) for k, v in args.items()}
    lo, hi = np.zeros((E, len(COLUMNS))), np.zeros((E, len(COLUMNS)))
    for e in range(E):
        for j, c in enumerate(COLUMNS):
            if c == "kind":
                box = (float(kinds[e]),) * 2
            else:
                x = slots[c][e]
                if x is None and c in ("t0_mjd", "log10_tau"):
                    if kinds[e] != 3:
                        raise ValueError(f"set_chromatic_event_prior: {c} is required for slot {e} of kind {KINDS[kinds[e]]!r}")
                    x = 0.0
                if c == "psr":
                    box = (0.0, float(P)) if x is None else _box(c, x, e)
                    if np.ndim(x) == 0 and x is not None and (box[0] != np.floor(box[0]) or not 0 <= box[0] <= P - 1):
                        raise ValueError(f"set_chromatic_event_prior: psr of slot {e} must be an integer in 0 .. P-1 = {P - 1}, got {x!r}")
                    if not (0 <= box[0] and box[1] <= P):
                        raise ValueError(f"set_chromatic_event_prior: psr of slot {e} must lie inside (0, P = {P}), got {x!r}")
                elif c == "log10_tau_pre":
                    box = (np.nan, np.nan) if x is None else _box(c, x, e, nan_ok=True)
                elif c == "sign":
                    box = (-1.0, 1.0) if isinstance(x, str) and x == "random" else _box(c, x, e)
                    if box == (0.0, 0.0):
                        raise ValueError(f"set_chromatic_event_prior: sign of slot {e} must be non-zero")
                else:
                    if x is None:
                        raise ValueError(f"set_chromatic_event_prior: {c} of slot {e} is required")
                    box = _box(c, x, e)
            lo[e, j], hi[e, j] = box
    return {"kind": np.array(kinds, dtype=np.int32), "lo": lo, "hi": hi}


def prior_bounds(prior):
    """lo, hi [E * 9] of pta_chrom_event_uniform for a make_prior() dict, slot-major"""
    return np.ascontiguousarray(prior["lo"]).ravel(), np.ascontiguousarray(prior["hi"]).ravel()


def labels(table):
    """{theta key: column} of the sampled event table [R, E, 9]; ce_psr and ce_kind as int32"""
    import torch
    out = {"ce_" + c: table[:, :, j].contiguous() for j, c in enumerate(COLUMNS)}
    out["ce_psr"], out["ce_kind"] = out["ce_psr"].to(torch.int32), out["ce_kind"].to(torch.int32)
    return out


# ---------------------------------------------------------------- NumPy evaluation (the list API, tests) -----------------------------
def event(toa_s, freqs_mhz, kind, log10_a, t0_mjd=0.0, log10_tau=0.0, log10_tau_pre=np.nan, sign=-1.0, index=2.0, phase=0.0,
          ref_freq_mhz=1400.0):
    """one event at the TOAs toa_s [s] with radio frequencies freqs_mhz: the definition as written, in the precision of toa_s"""
    t = np.asarray(toa_s)
    ft = t.dtype.type if t.dtype.kind == "f" else np.float64
    t = t.astype(ft)
    kind = kind_code(kind)
    amp = (-1 if float(sign) < 0 else 1) * ft(10) ** ft(log10_a) * (ft(ref_freq_mhz) / np.asarray(freqs_mhz, dtype=ft)) ** ft(index)
    if kind == 3:
        return amp * np.sin(8 * np.arctan(ft(1)) * t / ft(YEAR_IN_SEC) + ft(phase))
    dt, tau = t - ft(np.float64(t0_mjd) * 86400.0), ft(10) ** ft(log10_tau)
    if kind == 2:
        return amp * np.exp(-ft(0.5) * (dt / tau) ** 2)
    pre = tau if log10_tau_pre is None or np.isnan(log10_tau_pre) else ft(10) ** ft(log10_tau_pre)
    before = np.exp(-np.abs(dt) / pre) if kind == 1 else np.zeros_like(t)
    return amp * np.where(dt >= 0, np.exp(-np.abs(dt) / tau), before)


def term(toa_s, freqs_mhz, rows, ref_freq_mhz=1400.0):
    """the sum of the events `rows` (dicts over COLUMNS; psr is ignored, the optional columns take their defaults) at one pulsar's TOAs
    toa_s [s] with radio frequencies freqs_mhz, in ascending order: what add_chromatic_event records"""
    out = np.zeros(np.shape(toa_s), dtype=np.result_type(np.asarray(toa_s).dtype, np.float64))
    for row in rows:
        unknown = set(row) - set(COLUMNS)
        if unknown:
            raise ValueError(f"chromatic event: unknown column(s) {sorted(unknown)} (expected some of {list(COLUMNS)})")
        kw = {c: row[c] for c in COLUMNS[2:] if row.get(c) is not None}
        out = out + event(toa_s, freqs_mhz, row["kind"], ref_freq_mhz=ref_freq_mhz, **kw)
    return out
