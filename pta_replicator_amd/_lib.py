"""ctypes binding of libpta_replicator_amd.so (the C ABI declared in include/pta_replicator_amd.h).

There is no CPU fallback: if the shared library is missing the import fails loudly, and every entry
point raises ``PtaError`` with the library's own message on a non-zero return code.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p

# torch must own the HIP runtime of the process: it ships its own libamdhip64.so.7 and our library must
# bind to that same copy (same SONAME) so that tensors' device pointers and streams are valid inside it.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTA_REPLICATOR_AMD_LIB: an explicitly named build of the SAME library (probe builds with diagnostic defines: scripts/probe_src/) - never a fallback
LIB_PATH = os.environ.get("PTA_REPLICATOR_AMD_LIB") or os.path.join(_HERE, "libpta_replicator_amd.so")


class PtaError(RuntimeError):
    """A call into libpta_replicator_amd.so returned a PTA_E_* code."""


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build the HIP library first (python -m pta_replicator_amd.build, or "
        "__graft_entry__.build()). pta_replicator_amd has no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)

_P = c_void_p  # device / host raw pointers are passed as integers


class EnginePlan(ctypes.Structure):
    """pta_engine_plan (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_toa", c_int32), ("n_psr", c_int32), ("rn_k", c_int32), ("gw_npts", c_int32), ("tnequad", c_int32),
        ("n_tiles", c_int32),
        ("tile_psr", _P), ("tile_start", _P), ("tile_count", _P), ("tile_ep0", _P), ("tile_epn", _P),
        ("idx_in_psr", _P), ("Ft", _P), ("ldf", c_int64), ("rn_coef", _P), ("gw_G", _P),
        ("gw_jlo", _P), ("gw_w", _P), ("wn_a", _P), ("wn_b", _P), ("epoch_of", _P),
        ("ecorr_toa", _P), ("det", _P), ("wn_c", _P), ("rng_fast", c_int32), ("synth_variant", c_int32),
    ]


class EngineTables(ctypes.Structure):
    """pta_engine_tables (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("rn_amp", _P), ("Mchol", _P), ("gw_nf", c_int32), ("gw_i0", c_int32), ("use_czt", c_int32), ("czt_variant", c_int32),
        ("czt_pre", _P), ("czt_FB", _P), ("czt_tw", _P), ("czt_post", _P), ("Tsym", _P), ("rot", _P),
        ("ws_coef", _P), ("ws_G0", _P), ("ws_G", _P), ("idft_variant", c_int32), ("mix_variant", c_int32),
    ]


class TdPlan(ctypes.Structure):
    """pta_td_plan (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("Lbase", _P), ("blk_pos", _P), ("blk_ld", _P), ("blk_n", _P), ("blk_off", _P), ("item_blk", _P), ("item_n0", _P),
        ("n_blocks", c_int32), ("n_items", c_int32), ("rows_per_real", c_int32), ("stream_kind", c_uint32),
        ("rng_fast", c_int32), ("gw_npts", c_int32),
        ("gw_G", _P), ("gw_jlo", _P), ("gw_w", _P), ("det", _P), ("z", _P), ("ld_z", c_int64), ("blk_zoff", _P), ("item_rows", _P),
    ]


class EngineHyper(ctypes.Structure):
    """pta_engine_hyper (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("gw_scale", _P), ("ld_gw_scale", c_int64), ("gw_log10_A", _P), ("gw_gamma", _P), ("gw_f", _P), ("gw_hcf0", _P),
        ("gw_turnover", c_int32), ("gw_f0", c_double), ("gw_beta", c_double), ("gw_power", c_double), ("ws_scale", _P),
        ("rn_f", _P), ("rn_tspan", _P), ("rn_log10_A", _P), ("rn_gamma", _P), ("gw_mchol", _P), ("ld_gw_mchol", c_int64),
    ]


class CwEngine(ctypes.Structure):
    """pta_cw_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("mode", c_int32), ("psr_term", c_int32), ("amp_is_h", c_int32), ("has_pdist", c_int32), ("tref", c_double),
        ("phat", _P), ("pdist", _P), ("toa_s", _P), ("src", _P), ("ld_src", c_int64), ("par", _P),
    ]


class CwCatalogEngine(ctypes.Structure):
    """pta_cw_catalog_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("n_src", c_int32), ("mode", c_int32), ("psr_term", c_int32), ("amp_is_h", c_int32), ("has_pdist", c_int32),
        ("tref", c_double), ("phat", _P), ("pdist", _P), ("ld_pdist", c_int64), ("toa_s", _P), ("src", _P), ("ld_src", c_int64),
        ("count", _P), ("par", _P),
    ]


class BwmEngine(ctypes.Structure):
    """pta_bwm_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("phat", _P), ("toa_s", _P), ("src", _P), ("ld_src", c_int64), ("coef", _P), ("t0_s", _P),
    ]


class BurstEngine(ctypes.Structure):
    """pta_burst_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("n_wav", c_int32), ("phat", _P), ("toa_s", _P), ("sky", _P), ("src", _P), ("count", _P), ("wav", _P),
        ("kk", _P), ("psr_off", _P), ("quad_q", _P), ("quad_c", _P),
    ]


class TransientEngine(ctypes.Structure):
    """pta_transient_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("n_wav", c_int32), ("toa_s", _P), ("src", _P), ("count", _P), ("tab", _P),
    ]


class ChromEventEngine(ctypes.Structure):
    """pta_chrom_event_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("n_ev", c_int32), ("toa_s", _P), ("lnu", _P), ("src", _P), ("count", _P), ("tab", _P),
    ]


class WnHyper(ctypes.Structure):
    """pta_engine_wn_hyper (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("n_wn", c_int32), ("n_ec", c_int32), ("tnequad", c_int32), ("max_per_psr", c_int32),
        ("sigma", _P), ("wn_group", _P), ("ec_group", _P), ("wn_psr0", _P), ("ec_psr0", _P),
        ("efac_conf", _P), ("equad_conf", _P), ("ecorr_conf", _P),
        ("efac", _P), ("ld_efac", c_int64), ("log10_equad", _P), ("ld_equad", c_int64), ("log10_ecorr", _P), ("ld_ecorr", c_int64),
        ("ea", _P), ("eb", _P), ("ec", _P),
    ]


class ChromEngine(ctypes.Structure):
    """pta_chrom_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("k", c_int32), ("rng_fast", c_int32), ("Ft", _P), ("ldf", c_int64), ("amp", _P), ("f", _P), ("tspan", _P),
        ("log10_A", _P), ("gamma", _P), ("ld_theta", c_int64), ("coef", _P),
    ]


class PopPlan(ctypes.Structure):
    """pta_pop_plan (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_cells", c_int32), ("n_sorted", c_int32), ("n_bins", c_int32), ("k", c_int32), ("t_obs", c_double),
        ("cell_ptr", _P), ("number", _P), ("hs2", _P), ("fo", _P), ("orig", _P), ("log10_mc", _P), ("log10_fo", _P), ("log10_dl", _P),
    ]


class CprocEngine(ctypes.Structure):
    """pta_cproc_engine (include/pta_replicator_amd.h)."""
    _fields_ = [
        ("n_psr", c_int32), ("n_proc", c_int32), ("k", c_int32), ("rng_fast", c_int32), ("kp", c_int32 * 4), ("rho", c_int32 * 4), ("B", _P * 4),
        ("amp", _P), ("tspan", c_double), ("log10_A", _P), ("gamma", _P), ("ld_theta", c_int64), ("sc1", _P), ("coef", _P),
    ]


_SIGNATURES = {
    "pta_abi_version": (c_int, []),
    "pta_last_error": (c_char_p, []),
    "pta_device_info": (c_int, [POINTER(c_int), POINTER(c_int), c_char_p, c_int]),
    "pta_rng_philox_raw": (c_int, [_P, _P, c_int, _P, _P]),
    "pta_rng_fill_normal": (c_int, [c_uint64, c_uint64, c_int, c_uint32, c_int, c_int, _P, _P, c_int64, c_int, _P]),
    "pta_rng_fill_normal_blocks": (c_int, [c_uint64, c_uint64, c_int, c_uint32, c_int, _P, _P, c_int, _P, c_int64, c_int, _P]),
    "pta_rn_basis": (c_int, [_P, c_int, c_double, _P, _P, c_int, c_int, _P, c_int64, _P]),
    "pta_rn_synth": (c_int, [_P, c_int64, c_int, c_int, _P, c_int64, c_int, _P, c_int64, c_int, _P]),
    "pta_wn": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, c_int64, c_int, _P, c_int64, c_int, _P]),
    "pta_quantize_epochs": (c_int, [_P, c_int, c_double, _P, _P, _P, POINTER(c_int)]),
    "pta_dot3_host": (c_int, [_P, c_int64, _P, _P]),
    "pta_pow_host": (c_int, [_P, c_double, c_int64, _P]),
    "pta_legacy_randn": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, c_int]),
    "pta_ecorr": (c_int, [_P, _P, c_int, c_int, _P, c_int64, c_int, _P, c_int64, c_int, _P]),
    "pta_orf_pair_arguments": (c_int, [_P, c_int, _P, _P]),
    "pta_orf_hd": (c_int, [_P, c_int, _P, _P]),
    "pta_orf_basis": (c_int, [_P, _P, c_int, c_int, _P, _P]),
    "pta_orf_combine": (c_int, [_P, _P, c_int, c_int, _P, _P]),
    "pta_potrf_batched": (c_int, [_P, c_int, c_int, _P, _P]),
    "pta_potrf_batched_ex": (c_int, [_P, c_int, c_int64, c_int64, c_int, _P, c_int, _P]),
    "pta_potrf_workspace_doubles": (c_int64, [c_int, c_int, c_int]),
    "pta_potrf_batched_ws": (c_int, [_P, c_int, c_int64, c_int64, c_int, _P, c_int, _P, c_int64, _P]),
    "pta_potrf_warmup": (c_int, [c_int]),
    "pta_td_assemble_potrf": (c_int, [_P, _P, c_int, _P, _P, _P, _P, c_int, c_int64, c_int64, c_int, _P, c_int, _P, c_int64, _P]),
    "pta_potrf_ragged_plan_words": (c_int64, [c_int]),
    "pta_potrf_ragged_plan": (c_int, [_P, _P, _P, c_int, c_int, _P, POINTER(c_int64)]),
    "pta_potrf_ragged": (c_int, [_P, _P, _P, _P, _P, c_int64, _P]),
    "pta_gwb_twiddle": (c_int, [_P, c_int, c_int, c_int, c_double, _P, c_int64, _P]),
    "pta_gwb_idft": (c_int, [_P, c_int64, c_int, c_int, _P, c_int64, c_int, _P, c_int64, c_int, _P]),
    "pta_gwb_twiddle_sym_size": (c_int64, [c_int, c_int, c_int, POINTER(c_int64)]),
    "pta_gwb_twiddle_sym": (c_int, [_P, c_int, c_int, c_int, c_double, _P, _P, c_int, _P]),
    "pta_gwb_idft_rng": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, c_int, _P, c_int64, c_int, c_int, _P]),
    "pta_gwb_czt_fits": (c_int, [c_int, c_int, c_int]),
    "pta_gwb_czt_setup": (c_int, [_P, c_int, c_int, c_int, c_double, _P, _P, _P, _P, _P]),
    "pta_gwb_czt": (c_int, [c_uint64, c_uint64, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int64, c_int, c_int, _P]),
    "pta_gwb_czt_scaled": (c_int, [c_uint64, c_uint64, _P, c_int64, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int64, c_int, c_int,
                                   _P, c_int64, _P]),
    "pta_gwb_idft_rng_scaled": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, c_int, _P, c_int64, c_int, c_int, _P, c_int64, _P]),
    "pta_gwb_spectrum_scale": (c_int, [_P, _P, c_int, c_int, _P, _P, c_int, c_double, c_double, c_double, _P, c_int64, _P]),
    "pta_gwb_mix": (c_int, [_P, c_int, _P, c_int, c_int, c_int64, _P, c_int, _P]),
    "pta_gwb_orf_factor": (c_int, [_P, c_int, c_int, _P, c_int64, c_int, _P, _P, _P]),
    "pta_gwb_mix_batched": (c_int, [_P, c_int64, c_int, _P, c_int, c_int, c_int64, _P, c_int, _P]),
    "pta_gwb_bracket": (c_int, [_P, c_int, _P, c_int, _P, _P]),
    "pta_gwb_weights": (c_int, [_P, c_int, _P, _P, c_int, _P, _P]),
    "pta_gwb_interp": (c_int, [_P, c_int64, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_double, _P, c_int64, c_int, _P]),
    "pta_cgw": (c_int, [_P, c_int, _P, _P, c_int, _P]),
    "pta_cw_catalog_workspace": (c_int, [c_int, c_int, POINTER(c_int64), POINTER(c_int)]),
    "pta_cw_catalog": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_double, _P, _P, c_int, _P]),
    "pta_engine_rn_coef": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, c_int, _P]),
    "pta_engine_generate": (c_int, [POINTER(EnginePlan), POINTER(EngineTables), c_uint64, c_uint64, c_int, _P, c_int64, _P]),
    "pta_hyper_uniform": (c_int, [c_uint64, c_uint64, c_int, c_int, _P, _P, _P, _P]),
    "pta_engine_rn_coef_hyper": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "pta_engine_generate_hyper": (c_int, [POINTER(EnginePlan), POINTER(EngineTables), POINTER(EngineHyper), c_uint64, c_uint64, c_int, _P,
                                          c_int64, _P]),
    "pta_cw_uniform": (c_int, [c_uint64, c_uint64, c_int, c_int, _P, _P, _P, _P]),
    "pta_engine_cw_params": (c_int, [POINTER(CwEngine), c_int, _P]),
    "pta_engine_cw_add": (c_int, [POINTER(EnginePlan), POINTER(CwEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_cw_catalog_uniform": (c_int, [c_uint64, c_uint64, c_int, c_int, _P, _P, _P, _P]),
    "pta_engine_cw_catalog_params": (c_int, [POINTER(CwCatalogEngine), c_int, _P]),
    "pta_engine_cw_catalog_add": (c_int, [POINTER(EnginePlan), POINTER(CwCatalogEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_bwm_uniform": (c_int, [c_uint64, c_uint64, c_int, _P, _P, _P, _P]),
    "pta_engine_bwm_params": (c_int, [POINTER(BwmEngine), c_int, _P]),
    "pta_engine_bwm_add": (c_int, [POINTER(EnginePlan), POINTER(BwmEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_burst_uniform": (c_int, [c_uint64, c_uint64, c_int, c_int, _P, _P, _P, _P, _P]),
    "pta_transient_uniform": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, _P, _P]),
    "pta_engine_burst_params": (c_int, [POINTER(BurstEngine), c_int, _P]),
    "pta_engine_burst_quad": (c_int, [POINTER(BurstEngine), c_int, _P]),
    "pta_engine_burst_add": (c_int, [POINTER(EnginePlan), POINTER(BurstEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_engine_transient_params": (c_int, [POINTER(TransientEngine), c_int, _P]),
    "pta_engine_transient_add": (c_int, [POINTER(EnginePlan), POINTER(TransientEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_chrom_event_uniform": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, _P, _P]),
    "pta_engine_chrom_event_params": (c_int, [POINTER(ChromEventEngine), c_int, _P]),
    "pta_engine_chrom_event_add": (c_int, [POINTER(EnginePlan), POINTER(ChromEventEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_engine_wn_params": (c_int, [POINTER(WnHyper), c_int, _P]),
    "pta_engine_wn_add": (c_int, [POINTER(EnginePlan), POINTER(WnHyper), c_uint64, c_uint64, c_int, _P, c_int64, c_int, _P]),
    "pta_engine_chrom_coef": (c_int, [POINTER(ChromEngine), c_uint64, c_uint64, c_int, _P]),
    "pta_engine_chrom_add": (c_int, [POINTER(EnginePlan), POINTER(ChromEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_engine_cproc_coef": (c_int, [POINTER(CprocEngine), c_uint64, c_uint64, c_int, _P]),
    "pta_engine_cproc_add": (c_int, [POINTER(EnginePlan), POINTER(CprocEngine), c_int, _P, c_int64, c_int, _P]),
    "pta_engine_synth": (c_int, [POINTER(EnginePlan), c_uint64, c_uint64, c_int, _P, c_int64, _P]),
    "pta_td_cov_assemble": (c_int, [_P, c_int64, c_int, c_int, _P, _P, _P, _P, _P, c_int64, _P]),
    "pta_td_cov_assemble_all": (c_int, [_P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "pta_td_cov_walk_items": (c_int64, [_P, c_int, c_int, c_int, _P]),
    "pta_td_cov_assemble_walk": (c_int, [_P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_int64, _P, c_int, _P]),
    "pta_td_trmm": (c_int, [_P, c_int64, c_int, _P, c_int64, c_int, _P, c_int64, c_int, c_int, _P]),
    "pta_td_trmm_rng": (c_int, [POINTER(TdPlan), c_uint64, c_uint64, c_int, _P, c_int64, _P]),
    "pta_tm_project": (c_int, [_P, _P, c_int64, c_int, _P, c_int, _P, c_int64, c_int, _P]),
    "pta_os_project": (c_int, [_P, c_int64, c_int, _P, c_int, _P, c_int64, c_int, _P, c_int64, _P]),
    "pta_os_pairs": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, c_int64, _P, _P, c_int64, _P]),
    "pta_os_matched_prior": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_double, _P, _P, _P, _P, _P]),
    "pta_os_matched_solve": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P]),
    "pta_os_matched_pairs": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_int, _P, _P, c_int, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P]),
    "pta_os_pairs_pf": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, c_int, _P, c_int64, _P]),
    "pta_os_matched_pairs_pf": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_int, _P, _P, c_int, c_int, _P, c_int64, _P, c_int64, _P, c_int64, _P]),
    "pta_lnl_quad": (c_int, [_P, c_int64, c_int, _P, c_int, _P, _P, _P, _P, _P, _P, c_int64, c_int, c_int, c_int, _P, c_int64, _P, _P]),
    "pta_lnl_factor": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "pta_lnl_apply": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, c_int64, c_int, c_int, c_int, _P, _P, _P, _P, c_int64, c_int64, _P]),
    "pta_lnl_reduce": (c_int, [_P, c_int64, c_int64, c_int, c_int, c_int, _P, c_int64, _P]),
    "pta_clnl_mix": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, c_int, _P, c_int64, _P]),
    "pta_clnl_assemble": (c_int, [_P, c_int, c_int, c_double, c_double, _P, _P, c_int, _P, _P]),
    "pta_clnl_rhs": (c_int, [_P, c_int64, c_int, c_int, c_int, c_double, c_double, _P, _P, c_int, _P, c_int64, _P]),
    "pta_clnl_solve": (c_int, [_P, c_int, c_int, _P, c_int64, c_int, _P, c_int64, _P]),
    "pta_clnl_finish": (c_int, [_P, c_int, c_int, _P, c_int64, c_int, _P, c_int64, _P]),
    "pta_fstat_project": (c_int, [_P, c_int64, c_int, _P, c_int, _P, c_int64, c_int, _P, c_int64, _P]),
    "pta_fstat_fp": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, _P, c_int64, _P]),
    "pta_fstat_fe_tiles": (c_int64, [c_int]),
    "pta_fstat_fe": (c_int, [_P, c_int64, c_int, c_int, c_int, _P, c_int, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "pta_bwm_stat": (c_int, [_P, c_int64, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "pta_gather_rank0":(c_int, [_P, c_int, c_int, c_int, _P, c_int64, c_int64, c_int64, _P, c_int64, _P]),
    "pta_dgemm": (c_int, [c_int, c_int, c_int, c_int, c_double, _P, c_int64, c_int64, _P, c_int64, c_double, _P, c_int64,
                          c_int, c_int, c_int64, c_int64, c_int64, c_int, _P]),
    "pta_microbench": (c_int, [c_int, c_int64, c_int, c_int, POINTER(c_double)]),
    "pta_clock_probe": (c_int, [_P, c_int, c_int, c_int, _P]),
    "pta_selftest_mfma_f64": (c_int, [POINTER(c_double)]),
    "pta_pop_draw_select": (c_int, [POINTER(PopPlan), c_uint64, c_uint64, c_int, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, _P]),
    "pta_pop_theta": (c_int, [POINTER(PopPlan), c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _P]),
    "pta_os_project_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_lnl_apply_plan": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_fstat_project_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_gwb_mix_batched_plan": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_fstat_fe_plan": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_bwm_stat_plan": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_tm_project_plan": (c_int, [c_int, c_int, c_int, POINTER(c_int32)]),
    "pta_dgemm_plan": (c_int, [c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int,
                               POINTER(c_int32)]),
    "pta_gwb_spectrum_scale_user": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, c_int64, _P, c_int64, _P]),
    "pta_hyper_uniform_field": (c_int, [c_uint64, c_uint64, c_int, c_int, c_int, _P, _P, _P, _P]),
    "pta_os_matched_prior_spec": (c_int, [c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_double, _P, _P, _P, c_int, _P, c_int64, _P, _P, _P]),
}

# the values a pta_*_plan entry writes, in order (include/pta_replicator_amd.h)
_PLAN_FIELDS = {
    "pta_os_project": ("rw", "ct", "grid_x"),
    "pta_lnl_apply": ("kt", "g_per", "gz"),
    "pta_fstat_project": ("bm", "bn"),
    "pta_gwb_mix_batched": ("nta", "tpw", "grid_x"),
    "pta_fstat_fe": ("ks", "rchunk", "ngz"),
    "pta_bwm_stat": ("ks", "rchunk", "ngz"),
    "pta_tm_project": ("m", "grid_y"),
    "pta_dgemm": ("kernel", "tile", "lower_mode", "grid_x", "grid_y"),
}

# plan["kernel"] / plan["lower_mode"] of pta_dgemm_plan (include/pta_replicator_amd.h)
DGEMM_KERNELS = ("k_dgemm_valu<false>", "k_dgemm_valu<true>", "k_dgemm_mfma<false>", "k_dgemm_mfma<true>", "k_dgemm_mfma128<false,false>",
                 "k_dgemm_mfma128<true,false>", "k_dgemm_mfma128<true,true>", "k_dgemm_glds128<false,0>", "k_dgemm_glds128<false,1>")
DGEMM_LOWER = ("none", "grid2d", "triangle", "trapezoid")


def launch_plan(launcher, *sizes):
    """What `launcher` would choose for a launch of these sizes (the arguments of its pta_*_plan entry, without `plan`), as a dict.
    No device call."""
    out = (c_int32 * 8)()
    check(getattr(lib, launcher + "_plan")(*[int(v) for v in sizes], out), launcher + "_plan")
    return {k: int(out[i]) for i, k in enumerate(_PLAN_FIELDS[launcher])}


ENGINE_TILE = 256   # PTA_ENGINE_TILE
ENGINE_EPMAX = 132  # PTA_ENGINE_EPMAX
CW_ENGINE_NPAR = 16  # PTA_CW_ENGINE_NPAR
CW_CATALOG_NPAR = (16, 8, 8)  # by mode: PTA_CW_CATALOG_NPAR_EVOLVE, PTA_CW_CATALOG_NPAR_FOLDED (phase_approx, monochromatic)
WN_HYPER_GMAX = 16   # PTA_WN_HYPER_GMAX
CHROM_RG = 16        # PTA_CHROM_RG (csrc/pta_chrom.h): realisations per workgroup of pta_engine_chrom_add
CPROC_RG = 16        # PTA_CPROC_RG (csrc/pta_cproc.h): realisations per workgroup of pta_engine_cproc_add
CPROC_MAX = 4        # PTA_CPROC_MAX: common processes per engine
CPROC_KMAX = 64      # PTA_CPROC_KMAX: columns (2 x 32 frequencies)
OS_CMAX = 64         # PTA_OS_CMAX
OS_NORF = 8          # PTA_OS_NORF: ORFs (weight rows) of one pta_os_pairs call
OSM_KMAX = 128       # PTA_OSM_KMAX
LNL_KMAX = 128       # PTA_LNL_KMAX
LNL_MMAX = 16        # PTA_LNL_MMAX
CLNL_CMAX = 64       # PTA_CLNL_CMAX (csrc/pta_clnl.h)
CLNL_NORF = 4        # ORFs of one prepare_correlated_likelihood
CLNL_YMAX = 8192     # P * C doubles of one realisation's projections in the LDS of pta_clnl_mix
POP_KMAX = 128       # PTA_POP_KMAX: loudest cells kept per (realisation, frequency bin)
POP_FMAX = 64        # PTA_POP_FMAX
POP_CHUNK = 1024     # PTA_POP_CHUNK
FSTAT_CMAX = 4096    # PTA_FSTAT_CMAX
FSTAT_PMAX = 128     # PTA_FSTAT_PMAX
TD_STRIP = 256      # PTA_TD_STRIP
POTRF_ZERO_UPPER, POTRF_NO_LOOKAHEAD, POTRF_SUBSTITUTION, POTRF_VALU, POTRF_REG_STAGING, POTRF_LOCKSTEP, POTRF_DIAG_AHEAD, POTRF_DIAG64 = 1, 2, 4, 8, 32, 64, 128, 16
POTRF_EPI1 = 0x100000
POTRF_LEFT, POTRF_LEFT_SPLIT, POTRF_SOLVE_ROWS = 0x200000, 0x400000, 0x800000


def POTRF_CHAINS(c):
    """PTA_POTRF_CHAINS(c): number of concurrent chains of matrices of pta_potrf_batched_ex."""
    return (int(c) & 0xF) << 16


def POTRF_NB(k):
    """PTA_POTRF_NB(k): panel width override of pta_potrf_batched_ex, k * 256 columns."""
    return (int(k) & 0xFF) << 8

EXPORTS = tuple(_SIGNATURES)

for _name, (_res, _args) in _SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the .so is stale: rebuild
    _fn.restype = _res
    _fn.argtypes = _args

if lib.pta_abi_version() != 8:
    raise ImportError("libpta_replicator_amd.so has an unexpected ABI version: rebuild it")


def last_error():
    msg = lib.pta_last_error()
    return msg.decode() if msg else ""


def check(rc, what=""):
    if rc != 0:
        raise PtaError(f"{what or 'libpta_replicator_amd'} failed (code {rc}): {last_error()}")


def call(name, *args):
    """Call an int-returning entry point and raise on error."""
    check(getattr(lib, name)(*args), name)
