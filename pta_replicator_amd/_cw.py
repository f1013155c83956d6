"""One continuous-wave source per realisation (ReplicaEngine.set_cw): host-side validation, the column layout of the CW labels and
the strain <-> distance conversion.  Plain functions of the configuration and the arrays, so that they run (and are tested) without
a GPU, like _hyper.py.

theta may hold, next to the GWB / red-noise keys of _hyper,
    cw_cos_gwtheta, cw_gwphi, cw_log10_mc [Msun], cw_log10_fgw [Hz], cw_phase0, cw_psi, cw_cos_inc     [R]
    exactly one of cw_log10_h (strain) or cw_log10_dist [Mpc]                                          [R]
    cw_pdist [kpc] (optional; default: set_cw's pdist)                                                 [R, P]
as NumPy arrays or torch tensors.  If any CW key is given, all source keys must be.

A CATALOGUE of S >= 1 sources per realisation: the seven source keys and the amplitude key all of shape [R, S] (never a mix of [R]
and [R, S]); cw_pdist stays [R, P], a property of the pulsar shared by a realisation's sources.  Optional
    cw_count [R], integers 0 .. S: realisation r uses its first cw_count[r] sources; entries past the count are neither checked nor
    evaluated (they may be NaN).  Left out = S sources each.  Refused with [R] keys.
[R] keys keep the single-source kernels; [R, S] keys (S = 1 too) take pta_engine_cw_catalog_params / pta_engine_cw_catalog_add.
"""
import numpy as np

from ._hyper import _as_array, _xp
from .constants import MPC2S, SOLAR2S

SRC_KEYS = ("cw_cos_gwtheta", "cw_gwphi", "cw_log10_mc", "cw_log10_fgw", "cw_phase0", "cw_psi", "cw_cos_inc")
AMP_KEYS = ("cw_log10_h", "cw_log10_dist")
PDIST_KEY = "cw_pdist"
COUNT_KEY = "cw_count"
KEYS = SRC_KEYS + AMP_KEYS + (PDIST_KEY, COUNT_KEY)
MAX_SOURCES = 1 << 24   # the source index is the 24-bit field of the label stream (CW, s)

# label columns of the source table (pta_cw_uniform: stream kind 8, pair = column); "amp" is log10 h or log10 dist
COLUMNS = ("cos_gwtheta", "gwphi", "log10_mc", "log10_fgw", "amp", "phase0", "psi", "cos_inc")
N_SRC = len(COLUMNS)
PRIOR_DEFAULTS = {"cos_gwtheta": (-1.0, 1.0), "gwphi": (0.0, 2 * np.pi), "phase0": (0.0, 2 * np.pi), "psi": (0.0, np.pi),
                  "cos_inc": (-1.0, 1.0)}
PRIOR_KEYS = ("cos_gwtheta", "gwphi", "log10_mc", "log10_fgw", "log10_h", "log10_dist", "phase0", "psi", "cos_inc", "pdist")


def n_columns(P, pdist):
    """label columns per realisation: the 8 source columns, then pdist of every pulsar when it is per realisation."""
    return N_SRC + (P if pdist else 0)


def columns(P):
    """column range of every theta key in the [R, n_columns] source table (the amplitude key takes column 4)."""
    cols = {"cw_" + c: (j, j + 1) for j, c in enumerate(COLUMNS) if c != "amp"}
    cols["cw_log10_h"] = cols["cw_log10_dist"] = (4, 5)
    cols[PDIST_KEY] = (N_SRC, N_SRC + P)
    return cols


def split(theta):
    """(rest, cw): the CW keys of a theta dict and everything else."""
    if not isinstance(theta, dict):
        raise ValueError("theta must be a dict of per-realisation parameters")
    cw = {k: v for k, v in theta.items() if k in KEYS}
    rest = {k: v for k, v in theta.items() if k not in KEYS}
    return rest, cw


def make_config(P, psrTerm=True, evolve=True, phase_approx=False, tref=0.0, pdist=1.0):
    """validated set_cw() configuration."""
    pd = np.asarray(pdist, dtype=np.float64)
    if pd.ndim == 0:
        pd = np.full(P, float(pd))
    if pd.shape != (P,):
        raise ValueError(f"set_cw: pdist must be a scalar or one value per pulsar ({P}), got shape {np.shape(pdist)}")
    if not np.all(np.isfinite(pd)) or np.any(pd <= 0):
        raise ValueError("set_cw: pdist must be finite and > 0 [kpc]")
    tref = float(tref)
    if not np.isfinite(tref):
        raise ValueError("set_cw: tref must be finite [s]")
    return dict(psrTerm=bool(psrTerm), evolve=bool(evolve), phase_approx=bool(phase_approx), tref=tref, pdist=pd)


def mode(conf):
    """0 evolve, 1 phase_approx, 2 monochromatic (add_cgw's flags, deterministic.py:111-139)."""
    return 0 if conf["evolve"] else (1 if conf["phase_approx"] else 2)


def check_theta(cw, R, P, conf, check_values=True):
    """validate the CW keys of theta for R realisations of a P-pulsar array; returns {key: array} (the caller's arrays, unconverted).
    check_values=False skips the value checks (labels drawn by pta_cw_uniform inside a validated prior)."""
    if not cw:
        return {}
    if conf is None:
        raise ValueError("theta: no per-realisation CW configured (set_cw)")
    missing = [k for k in SRC_KEYS if k not in cw]
    if missing:
        raise ValueError(f"theta: CW keys need every source key; missing {missing}")
    amp = [k for k in AMP_KEYS if k in cw]
    if len(amp) != 1:
        raise ValueError(f"theta: exactly one of {list(AMP_KEYS)} is needed, got {amp}")
    out = {k: _as_array(k, v) for k, v in cw.items() if k != COUNT_KEY}
    ndim = {k: len(tuple(v.shape)) for k, v in out.items() if k != PDIST_KEY}
    if set(ndim.values()) == {2}:      # a catalogue: [R, S]
        S = int(out[SRC_KEYS[0]].shape[1])
        if not 1 <= S <= MAX_SOURCES:
            raise ValueError(f"theta: a catalogue needs 1 <= S <= {MAX_SOURCES} sources per realisation, got shape {tuple(out[SRC_KEYS[0]].shape)}")
        src_shape = (R, S)
    elif 2 in ndim.values() and 1 in ndim.values():
        raise ValueError("theta: CW keys mix the shapes [R] and [R, S]: " + ", ".join(f"{k} {tuple(out[k].shape)}" for k in ndim))
    else:
        S, src_shape = None, (R,)
    for k, v in out.items():
        want = (R, P) if k == PDIST_KEY else src_shape
        if tuple(v.shape) != want:
            raise ValueError(f"theta[{k!r}]: shape {tuple(v.shape)}, expected {want}")
    count = None
    if COUNT_KEY in cw:
        if S is None:
            raise ValueError(f"theta[{COUNT_KEY!r}]: needs a catalogue (source keys of shape [R, S]); the source keys are [R]")
        count = out[COUNT_KEY] = check_count(cw[COUNT_KEY], R, S)
    if not check_values:
        return out
    live = None if count is None else _live(count, S)   # [R, S]: source s of realisation r is below the count
    for k, v in out.items():
        if k == COUNT_KEY:
            continue
        xp = _xp(v)
        bad = ~xp.isfinite(v)
        if live is not None and k != PDIST_KEY:
            bad = bad & _like(live, v)
        if bool(bad.any()):
            raise ValueError(f"theta[{k!r}]: non-finite values")
    for k in ("cw_cos_gwtheta", "cw_cos_inc"):
        bad = abs(out[k]) > 1
        if live is not None:
            bad = bad & _like(live, out[k])
        if bool(bad.any()):
            raise ValueError(f"theta[{k!r}]: |cos| > 1")
    if PDIST_KEY in out and bool((out[PDIST_KEY] <= 0).any()):
        raise ValueError(f"theta[{PDIST_KEY!r}]: pdist must be > 0 [kpc]")
    return out


def check_count(count, R, S):
    """cw_count validated: an integer array or tensor [R] with 0 <= count <= S (returned as given, unconverted)."""
    c = count if isinstance(count, np.ndarray) or hasattr(count, "device") else np.asarray(count)
    if _xp(c) is np:
        integer = c.dtype.kind in "iu"
    else:
        integer = not (c.dtype.is_floating_point or c.dtype.is_complex) and str(c.dtype) != "torch.bool"
    if not integer:
        raise ValueError(f"theta[{COUNT_KEY!r}]: expected an integer array, got dtype {c.dtype}")
    if tuple(c.shape) != (R,):
        raise ValueError(f"theta[{COUNT_KEY!r}]: shape {tuple(c.shape)}, expected {(R,)}")
    if bool((c < 0).any()) or bool((c > S).any()):
        raise ValueError(f"theta[{COUNT_KEY!r}]: counts must lie in 0 .. S = {S}")
    return c


def _live(count, S):
    """[R, S] mask (NumPy): source s of realisation r is in use."""
    c = count.cpu().numpy() if hasattr(count, "cpu") else np.asarray(count)
    return np.arange(S)[None, :] < c[:, None]


def _like(mask, v):
    """a NumPy mask as the array type of v"""
    if _xp(v) is np:
        return mask
    import torch
    return torch.as_tensor(mask, device=v.device)


def n_sources(cw):
    """sources per realisation of validated CW keys: 0 without CW keys, 1 for [R] keys, S for a catalogue [R, S].  The dict may hold
    other deterministic keys (bwm_*) next to them, or alone."""
    if not has_keys(cw):
        return 0
    shape = tuple(cw[SRC_KEYS[0]].shape)
    return int(shape[1]) if len(shape) == 2 else 1


def is_catalog(cw):
    return has_keys(cw) and len(tuple(cw[SRC_KEYS[0]].shape)) == 2


def has_keys(det):
    """True if a dict of validated deterministic keys (cw_* and bwm_*) holds a CW source."""
    return bool(det) and SRC_KEYS[0] in det


def amp_key(cw):
    return "cw_log10_h" if "cw_log10_h" in cw else "cw_log10_dist"


def log10_h_from_dist(log10_mc, log10_fgw, log10_dist):
    """strain h = 2 mc^(5/3) (pi fgw)^(2/3) / dist (geometric units: mc, dist in seconds)."""
    mc = 10.0 ** np.asarray(log10_mc, dtype=np.float64) * SOLAR2S
    w0 = np.pi * 10.0 ** np.asarray(log10_fgw, dtype=np.float64)
    dist = 10.0 ** np.asarray(log10_dist, dtype=np.float64) * MPC2S
    return np.log10(2 * mc ** (5 / 3) * w0 ** (2 / 3) / dist)


def log10_dist_from_h(log10_mc, log10_fgw, log10_h):
    """dist [Mpc] = 2 mc^(5/3) (pi fgw)^(2/3) / h."""
    mc = 10.0 ** np.asarray(log10_mc, dtype=np.float64) * SOLAR2S
    w0 = np.pi * 10.0 ** np.asarray(log10_fgw, dtype=np.float64)
    h = 10.0 ** np.asarray(log10_h, dtype=np.float64)
    return np.log10(2 * mc ** (5 / 3) * w0 ** (2 / 3) / h / MPC2S)


def make_prior(P, n_sources=None, **boxes):
    """validated set_cw_prior() boxes: {column name: (lo [n], hi [n])} plus "amp_is_h" and "n_sources".  log10_mc, log10_fgw and one of
    log10_h / log10_dist are required; the angles default to the isotropic boxes; pdist is optional, (lo, hi) or [P, 2].  n_sources:
    None = one source, labels [R]; S >= 1 = a catalogue of S independent draws from the same boxes, labels [R, S]."""
    if n_sources is not None:
        if isinstance(n_sources, bool) or not isinstance(n_sources, (int, np.integer)) or not 1 <= n_sources <= MAX_SOURCES:
            raise ValueError(f"set_cw_prior: n_sources must be an integer in 1 .. {MAX_SOURCES} (or None), got {n_sources!r}")
        n_sources = int(n_sources)
    unknown = set(boxes) - set(PRIOR_KEYS)
    if unknown:
        raise ValueError(f"set_cw_prior: unknown parameter(s) {sorted(unknown)} (expected some of {list(PRIOR_KEYS)})")
    for k in ("log10_mc", "log10_fgw"):
        if boxes.get(k) is None:
            raise ValueError(f"set_cw_prior: {k} is required")
    amp = [k for k in ("log10_h", "log10_dist") if boxes.get(k) is not None]
    if len(amp) != 1:
        raise ValueError("set_cw_prior: exactly one of log10_h / log10_dist is required")
    prior = {"amp_is_h": amp[0] == "log10_h", "n_sources": n_sources}
    for k in PRIOR_KEYS:
        box = boxes.get(k, None)
        if box is None:
            box = PRIOR_DEFAULTS.get(k)
        if box is None:
            continue
        b = np.asarray(box, dtype=np.float64)
        n = P if k == "pdist" else 1
        if b.shape == (2,):
            b = np.broadcast_to(b, (n, 2))
        if b.shape != (n, 2):
            raise ValueError(f"set_cw_prior: {k} must be (lo, hi){'' if n == 1 else f' or [{P}, 2]'}, got shape {np.shape(box)}")
        if not np.all(np.isfinite(b)) or np.any(b[:, 1] < b[:, 0]):
            raise ValueError(f"set_cw_prior: {k} needs finite bounds with lo <= hi")
        if k.startswith("cos_") and np.any(np.abs(b) > 1):
            raise ValueError(f"set_cw_prior: {k} must lie inside [-1, 1]")
        if k == "pdist" and np.any(b[:, 0] <= 0):
            raise ValueError("set_cw_prior: pdist must be > 0 [kpc]")
        prior["amp" if k in ("log10_h", "log10_dist") else k] = (b[:, 0].copy(), b[:, 1].copy())
    return prior


def prior_bounds(prior, P):
    """lo, hi [n_columns] of pta_cw_uniform for a make_prior() dict."""
    pd = "pdist" in prior
    lo, hi = np.zeros(n_columns(P, pd)), np.zeros(n_columns(P, pd))
    for j, c in enumerate(COLUMNS):
        lo[j], hi[j] = prior[c][0][0], prior[c][1][0]
    if pd:
        lo[N_SRC:], hi[N_SRC:] = prior["pdist"]
    return lo, hi


def labels(table, prior, P, catalog=None):
    """{theta key: view of the [R, n_columns] table} of sampled labels.  catalog: the [R, S, 8] table of pta_cw_catalog_uniform for a
    prior with n_sources = S; the source labels are then [R, S] and `table` is read for its pdist columns alone."""
    out = {}
    for j, c in enumerate(COLUMNS):
        k = ("cw_log10_h" if prior["amp_is_h"] else "cw_log10_dist") if c == "amp" else "cw_" + c
        out[k] = (table[:, j] if catalog is None else catalog[:, :, j]).contiguous()
    if "pdist" in prior:
        out[PDIST_KEY] = table[:, N_SRC:N_SRC + P].contiguous()
    return out


def pulsar_vectors(ra_dec_list):
    """[P, 3] unit vectors with the reference's expression: ptheta = pi/2 - dec, pphi = ra (deterministic.py:42-43, :88)."""
    out = np.zeros((len(ra_dec_list), 3))
    for a, (ra, dec) in enumerate(ra_dec_list):
        ptheta, pphi = np.pi / 2 - dec, ra
        out[a] = [np.sin(ptheta) * np.cos(pphi), np.sin(ptheta) * np.sin(pphi), np.cos(ptheta)]
    return out

