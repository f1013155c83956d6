"""ISA-level instruction-class table of the fused synthesis kernel (VERDICT r2 #3iii): where the ~219 VALU wave-instructions per output
element of k_engine_synth_mfma<false> go.  No GPU needed: hipcc --save-temps for gfx950, then

  * the Gaussian draw is compiled piece by piece (one tiny kernel per device function of pta_rng.h, inputs loaded from memory so that
    nothing folds away): Philox-4x32-10, the uniform conversion, -2 ln u, sqrt, sin/cos(2 pi u), the final products - exact static
    VALU / SALU / LDS counts of straight-line code;
  * the kernel itself is split at its basic blocks: ECORR staging loop (executed ~epn * 16 / 256 times per workgroup), red-noise
    MFMA loop (5 trips at K = 60), the unrolled 4-TOA epilogue (once) - static counts weighted by those trip counts give the
    dynamic VALU count per workgroup and per output element (16 realisations x 256 TOAs).

  * both addressings of the red-noise loop (template parameter RNIDX of the kernel) are listed side by side, and the chirp-z kernel
    k_gwb_czt<true, false, FUSE, false> is counted for the fused step 15, each of the bits 16 / 32 / 64 alone, the default and all three, with
    the twiddle and butterfly pieces those bits remove compiled on their own like the pieces of the draw.

  * RNIDX = true (unless SINGLE) also means two pairs of adjacent TOAs per lane: in a full tile the red-noise loop loads the design matrix
    16 bytes at a time (the loop copies with 9 memory instructions per trip; the copies with 15 serve a tile cut short), and the results
    leave as 16-byte stores.  The copy for complete plans (ALL = true, the one the bench workload runs) is listed and estimated as well,
    and every instance's registers, scratch and LDS, for this build and for the library's own (with the per-TOA ECORR path).

Writes profiles/r17_isa_instruction_classes.txt (r13_isa_instruction_classes.txt is the table before the adjacent-TOA mapping,
r03_isa_instruction_classes.txt the kernel as it was in round 3).  The PMC figure to compare with is SQ_INSTS_VALU / (R * n_toa / 64) of
profiles/r17_synth_wide.json."""
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pta_replicator_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result", "--save-temps", "-c"]

PROBE = r'''
#include <hip/hip_runtime.h>
#include "%(csrc)s/pta_rng.h"
#include "%(csrc)s/pta_fft.h"
extern "C" {
// chirp-z pieces: eight complex inputs per thread from memory, eight (or two) complex results back
#define P_LOADV(v) pta_cplx v[8]; for (int q = 0; q < 8; ++q) v[q] = ((const pta_cplx *)in)[8 * threadIdx.x + q]
#define P_STOREV(v, n) for (int q = 0; q < n; ++q) ((pta_cplx *)out)[8 * threadIdx.x + q] = v[q]
__global__ void p_c_empty(const double *in, double *out) { P_LOADV(v); P_STOREV(v, 8); }
__global__ void p_c_twiddles(const double *in, double *out) { pta_cplx w[8]; w[0] = {1.0, 0.0}; pta_fft_twiddles<9, 1>(in, threadIdx.x, w); P_STOREV(w, 8); }
__global__ void p_c_load1(const double *in, double *out) { pta_cplx w[8]; for (int q = 0; q < 8; ++q) w[q] = ((const pta_cplx *)in)[threadIdx.x]; P_STOREV(w, 8); }
__global__ void p_c_products(const double *in, double *out) { P_LOADV(w); pta_fft_twiddle_products(w); P_STOREV(w, 8); }
__global__ void p_c_dft8_inv(const double *in, double *out) { P_LOADV(v); pta_dft8<true>(v); P_STOREV(v, 8); }
__global__ void p_c_dft8_inv01(const double *in, double *out) { P_LOADV(v); pta_dft8_inv_out01(v); P_STOREV(v, 8); }
__global__ void p_philox(const uint32_t *in, uint32_t *out) {
  pta_u32x4 v = pta_philox_draw(((const uint64_t *)in)[0], ((const uint64_t *)in)[1] + threadIdx.x, in[4], in[5] + threadIdx.x);
  out[4 * threadIdx.x] = v.x; out[4 * threadIdx.x + 1] = v.y; out[4 * threadIdx.x + 2] = v.z; out[4 * threadIdx.x + 3] = v.w;
}
__global__ void p_uniform(const uint32_t *in, double *out) {
  pta_u32x4 v = {in[4 * threadIdx.x], in[4 * threadIdx.x + 1], in[4 * threadIdx.x + 2], in[4 * threadIdx.x + 3]};
  double a, b; pta_uniform_pair(v, a, b); out[2 * threadIdx.x] = a; out[2 * threadIdx.x + 1] = b;
}
__global__ void p_neg2log(const double *in, double *out) { pta_rng_stage_tables(); __syncthreads(); out[threadIdx.x] = pta_neg2log(in[threadIdx.x]); }
__global__ void p_sqrt(const double *in, double *out) { out[threadIdx.x] = pta_sqrt_pos(in[threadIdx.x]); }
__global__ void p_sincos(const double *in, double *out) {
  pta_rng_stage_tables(); __syncthreads();
  double s, c; pta_sincos_2pi(in[threadIdx.x], s, c); out[2 * threadIdx.x] = s; out[2 * threadIdx.x + 1] = c;
}
__global__ void p_pair(const uint32_t *in, double *out) {
  pta_rng_stage_tables(); __syncthreads();
  double a, b; pta_normal_pair(((const uint64_t *)in)[0], ((const uint64_t *)in)[1] + threadIdx.x, in[4], in[5] + threadIdx.x, a, b, 0);
  out[2 * threadIdx.x] = a; out[2 * threadIdx.x + 1] = b;
}
__global__ void p_empty_tables(const double *in, double *out) { pta_rng_stage_tables(); __syncthreads(); out[threadIdx.x] = in[threadIdx.x]; }
__global__ void p_empty(const double *in, double *out) { out[threadIdx.x] = in[threadIdx.x]; }
}
'''


def classify(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_"): return "valu"
    if op.startswith("s_waitcnt") or op.startswith("s_nop") or op.startswith("s_barrier"): return "wait"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    return "other"


def kernel_bodies(asm):
    out, name, body = {}, None, []
    for line in open(asm):
        m = re.match(r"^([A-Za-z_][\w]*):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            if name: out[name] = body
            name, body = m.group(1), []
            continue
        if name is None: continue
        if line.startswith(".Lfunc_end"):
            out[name] = body; name = None; continue
        body.append(line)
    return out


def count(lines):
    c, vops = collections.Counter(), collections.Counter()
    for ln in lines:
        t = ln.strip()
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"): continue
        op = t.split()[0]
        k = classify(op)
        c[k] += 1
        if k == "valu": vops[op] += 1
    return c, vops


def blocks(lines):
    """[(label, lines)] split at .LBB labels"""
    out, lab, cur = [], "entry", []
    for ln in lines:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            out.append((lab, cur)); lab, cur = m.group(1), []
        else:
            cur.append(ln)
    out.append((lab, cur))
    return out


def main():
    rep = []
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.hip")
        open(src, "w").write(PROBE % {"csrc": CSRC})
        subprocess.check_call([HIPCC] + FLAGS + [src, "-o", os.path.join(d, "probe.o")], cwd=d, stderr=subprocess.DEVNULL)
        kb = kernel_bodies(os.path.join(d, "probe-hip-amdgcn-amd-amdhsa-gfx950.s"))
        base = {k: count(kb[k])[0] for k in ("p_empty", "p_empty_tables")}
        rep.append("Gaussian draw, piece by piece (static counts of straight-line code; probe overhead - loads, address arithmetic, table staging - subtracted)")
        rep.append(f"{'piece':34s} {'VALU':>6s} {'LDS':>5s} {'SALU':>5s}   VALU mix (top)")
        tot = collections.Counter()
        for k, label, b in (("p_philox", "Philox-4x32-10 (counter -> 4 x u32)", "p_empty"), ("p_uniform", "2 x 52-bit uniform", "p_empty"),
                            ("p_neg2log", "-2 ln u (128-entry table + deg-5)", "p_empty_tables"), ("p_sqrt", "sqrt (rsq + Newton + residual)", "p_empty"),
                            ("p_sincos", "sin, cos 2 pi u (32-entry table + Taylor)", "p_empty_tables"), ("p_pair", "pta_normal_pair, whole (z0, z1)", "p_empty_tables")):
            c, vops = count(kb[k])
            v, l, s = c["valu"] - base[b]["valu"], c["lds"] - base[b]["lds"], c["salu"] - base[b]["salu"]
            top = ", ".join(f"{op} {n}" for op, n in vops.most_common(5))
            rep.append(f"{label:34s} {v:6d} {l:5d} {s:5d}   {top}")
            if k != "p_pair": tot["valu"] += v
        rep.append(f"{'sum of the pieces (+ 2 final products)':34s} {tot['valu'] + 2:6d}")
        # ---- the kernel itself
        subprocess.check_call([HIPCC] + FLAGS + ["-DPTA_ISA_TABLE_MAIN_PATH_ONLY", os.path.join(CSRC, "pta_engine_kernels.hip"), "-o", os.path.join(d, "eng.o")],
                              cwd=d, stderr=subprocess.DEVNULL)
        kb = kernel_bodies(os.path.join(d, "pta_engine_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"))
        def kernel_rows(name, title):
            rep.append("")
            rep.append(f"{title} ({name}): basic blocks with VALU / MFMA / LDS / VMEM counts")
            rows = []
            for lab, ls in blocks(kb[name]):
                c, vops = count(ls)
                if sum(c.values()) == 0: continue
                back = any(re.search(r"s_cbranch\w*\s+" + re.escape(lab) + r"\b", x) for x in ls)
                rows.append((lab, c, back, vops))
                rep.append(f"  {lab:12s} valu {c['valu']:5d}  mfma {c['mfma']:3d}  lds {c['lds']:3d}  vmem {c['vmem']:3d}  salu {c['salu']:4d}  wait {c['wait']:3d}{'   <- loop' if back else ''}")
            return rows

        def mix(vops):
            mul = sum(n for op, n in vops.items() if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64")))
            w64 = sum(n for op, n in vops.items() if op.endswith("_u64") or op.endswith("_b64") or op.endswith("_i64")) - sum(n for op, n in vops.items() if op.startswith("v_mad_"))
            return f"integer multiplies {mul}, other 64-bit integer {w64}: " + ", ".join(f"{op} {n}" for op, n in vops.most_common(8))

        # the red-noise loop with the per-lane 64-bit index products (RNIDX = false: synth_variant 2, the kernel before the change) ...
        old_rows = kernel_rows(next(k for k in kb if k.startswith("_Z19k_engine_synth_mfmaILb0ELb0ELb0ELb0E")), "k_engine_synth_mfma<false, false, false>")
        old_rn = [r for r in old_rows if r[2] and r[1]["mfma"] > 0]
        # ... and with scalar row offsets (RNIDX = true, default): two copies of the loop, K % 4 == 0 (fewer VALU: the bench's K = 60) and K % 4 != 0
        name = next(k for k in kb if k.startswith("_Z19k_engine_synth_mfmaILb0ELb0ELb1ELb0E"))
        rows = kernel_rows(name, "k_engine_synth_mfma<false, false, true, false>")
        all_rows = kernel_rows(next(k for k in kb if k.startswith("_Z19k_engine_synth_mfmaILb0ELb0ELb1ELb1E")),
                               "k_engine_synth_mfma<false, false, true, true> (the copy for complete plans: the bench workload's)")
        # four copies of the loop: 16-byte loads (full tile: fewer memory instructions) or 8-byte loads (tile cut short), K % 4 == 0 or not
        def loops(rs):
            rn = [r for r in rs if r[2] and r[1]["mfma"] > 0]
            wide = sorted((r for r in rn if r[1]["vmem"] == min(x[1]["vmem"] for x in rn)), key=lambda r: r[1]["valu"])
            narrow = sorted((r for r in rn if r not in wide), key=lambda r: r[1]["valu"])
            return rn, wide, narrow
        rn_all, new_rn, narrow_rn = loops(rows)
        rep.append("")
        rep.append("red-noise MFMA loop, per trip of 12 bins (3 K-steps):")
        for title, r in [("per-lane 64-bit index products (synth_variant 2), 8-byte loads", old_rn[0]),
                         ("scalar row offsets, K % 4 == 0, 8-byte loads (tile cut short)", narrow_rn[0]),
                         ("scalar row offsets, K % 4 != 0, 8-byte loads (tile cut short)", narrow_rn[-1]),
                         ("scalar row offsets, K % 4 == 0, 16-byte loads (default)", new_rn[0]),
                         ("scalar row offsets, K % 4 != 0, 16-byte loads", new_rn[-1])]:
            rep.append(f"  {title:66s} {r[0]:10s} valu {r[1]['valu']:3d} salu {r[1]['salu']:3d} vmem {r[1]['vmem']:3d}   {mix(r[3])}")
        rep.append(f"  static VALU of the kernel, per thread: {sum(r[1]['valu'] for r in old_rows)} (synth_variant 2), {sum(r[1]['valu'] for r in rows)} (default; holds all four copies of the loop)")
        keep = new_rn[0][0]
        rows = [r for r in rows if not (r in rn_all and r[0] != keep)]   # the dynamic estimate below takes the copy the bench workload runs
        rn_a, wide_a, _ = loops(all_rows)
        all_rows = [r for r in all_rows if not (r in rn_a and r[0] != wide_a[0][0])]
        # dynamic estimate: loops = blocks that branch back to themselves.  Identify them by content: the staging loop holds the
        # Philox multiplies (v_mad_u64_u32) and LDS writes but no MFMA; the red-noise loop holds MFMAs
        stag = [r for r in rows if r[2] and r[1]["mfma"] == 0 and r[1]["valu"] > 50]
        rnl = [r for r in rows if r[2] and r[1]["mfma"] > 0]
        once = sum(r[1]["valu"] for r in rows if not r[2])
        n_epochs_pairs = 121.0     # pairs a 256-TOA tile of the bench workload stages on average (4700 epochs per 5000 TOAs)
        t_stag = n_epochs_pairs * 16 / 256.0
        t_rn = 5.0                 # K = 60 in steps of 12
        dyn = once + sum(r[1]["valu"] for r in stag) * t_stag + sum(r[1]["valu"] for r in rnl) * t_rn
        per_elem = dyn / 16.0                # a wave writes 16 realisations x 64 TOAs: 16 output elements per lane
        rep.append("")
        rep.append(f"dynamic VALU wave-instructions per wave: straight-line {once} + staging loop {sum(r[1]['valu'] for r in stag)} x {t_stag:.2f} trips "
                   f"+ red-noise loop {sum(r[1]['valu'] for r in rnl)} x {t_rn:.0f} trips = {dyn:.0f}")
        rep.append(f"=> {per_elem:.1f} VALU instructions per output element (a wave writes 16 realisations x 64 TOAs = 16 elements per lane); "
                   f"the all-VALU alternatives of the has_gw / has_wn / epn branches are counted once each, so this is an upper bound of the executed path")
        pair = count(kernel_bodies(os.path.join(d, "probe-hip-amdgcn-amd-amdhsa-gfx950.s"))["p_pair"])[0]["valu"] - base["p_empty_tables"]["valu"]
        rng = (1 + n_epochs_pairs / 256.0) * pair
        rep.append(f"of which Gaussian draws: (1 EFAC/EQUAD pair + {n_epochs_pairs / 256.0:.3f} ECORR pairs) per element x {pair} = {rng:.1f} "
                   f"({100 * rng / per_elem:.0f} %); the remaining {per_elem - rng:.1f} are GWB interpolation, accumulation, operand addressing, MFMA feeding and stores")
        rep.append("per Gaussian pair: Philox 46 (20 of them v_mad_u64_u32 at half rate), uniforms 10, -2 ln u 22, sqrt 10, sin / cos 26, products 2")
        old_dyn = sum(r[1]["valu"] for r in old_rows if not r[2]) + sum(r[1]["valu"] for r in old_rows if r[2] and r[1]["mfma"] == 0 and r[1]["valu"] > 50) * t_stag + old_rn[0][1]["valu"] * t_rn
        rep.append(f"the same estimate with the per-lane index products: {old_dyn:.0f} per wave, {old_dyn / 16.0:.1f} per output element ({100 * (old_dyn - dyn) / old_dyn:.1f} % more)")
        a_once = sum(r[1]["valu"] for r in all_rows if not r[2])
        a_stag = sum(r[1]["valu"] for r in all_rows if r[2] and r[1]["mfma"] == 0 and r[1]["valu"] > 50)
        a_rn = sum(r[1]["valu"] for r in all_rows if r[2] and r[1]["mfma"] > 0)
        a_dyn = a_once + a_stag * t_stag + a_rn * t_rn
        a_mem = sum(r[1]["vmem"] for r in all_rows if not r[2]) + sum(r[1]["vmem"] for r in all_rows if r[2] and r[1]["mfma"] > 0) * t_rn
        rep.append(f"the copy for complete plans: straight-line {a_once} + staging loop {a_stag} x {t_stag:.2f} + red-noise loop {a_rn} x {t_rn:.0f} = {a_dyn:.0f} per wave, "
                   f"{a_dyn / 16.0:.1f} per output element; global-memory instructions per wave (both store paths and the loop prologues of all copies counted): {a_mem:.0f}")
        # ---- every instance's resources, in this build and in the library's own
        def resources(asm):
            meta = open(asm).read()
            out = {}
            for m in re.finditer(r"\.amdhsa_kernel (_Z19k_engine_synth_mfmaILb(\d)ELb(\d)ELb(\d)ELb(\d)E\S*)(.*?)\.end_amdhsa_kernel", meta, re.S):
                g = lambda key: int(re.search(key + r"\s+(\d+)", m.group(6)).group(1))
                out[tuple(int(m.group(i)) for i in (2, 3, 4, 5))] = (g("amdhsa_next_free_vgpr"), g("amdhsa_next_free_sgpr"), g("amdhsa_private_segment_fixed_size"),
                                                                    g("amdhsa_group_segment_fixed_size"))
            return out
        res_tab = resources(os.path.join(d, "pta_engine_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"))
        os.makedirs(os.path.join(d, "lib"))
        subprocess.check_call([HIPCC] + FLAGS + [os.path.join(CSRC, "pta_engine_kernels.hip"), "-o", os.path.join(d, "lib", "eng.o")], cwd=os.path.join(d, "lib"),
                              stderr=subprocess.DEVNULL)
        res_lib = resources(os.path.join(d, "lib", "pta_engine_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"))
        rep.append("")
        rep.append("k_engine_synth_mfma<FAST, SINGLE, RNIDX, ALL>: next free VGPR / next free SGPR / scratch bytes per lane / LDS bytes (128 VGPRs = 4 workgroups per CU; SINGLE is compiled for 3)")
        rep.append("FAST SINGLE RNIDX ALL    this table's build (staged-ECORR path only)    the library's build")
        for key in sorted(res_tab):
            a, b = res_tab[key], res_lib[key]
            rep.append(f"   {key[0]}      {key[1]}     {key[2]}   {key[3]}    {a[0]:4d} / {a[1]:3d} / {a[2]:3d} / {a[3]:6d}                      {b[0]:4d} / {b[1]:3d} / {b[2]:3d} / {b[3]:6d}")
        # ---- the chirp-z kernel
        rep.append("")
        rep.append("k_gwb_czt<true, false, FUSE, false>: static counts per thread (FUSE & 64 holds the full AND the pruned last butterfly: a launch runs one of them)")
        subprocess.check_call([HIPCC] + FLAGS + [os.path.join(CSRC, "pta_czt_kernels.hip"), "-o", os.path.join(d, "czt.o")], cwd=d, stderr=subprocess.DEVNULL)
        asm = os.path.join(d, "pta_czt_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")
        kc = kernel_bodies(asm)
        meta = open(asm).read()
        for fuse, what in ((15, "fused kernel (variant 25, before)"), (15 + 16, "+ s = 512 twiddle set carried in registers"), (15 + 32, "+ s = 8 / s = 64 sets from the LDS table"),
                           (15 + 64, "+ pruned last butterfly"), (15 + 16 + 64, "carried set + pruned butterfly (variant 0)"), (127, "all three (variant 137)")):
            kn = f"_Z9k_gwb_cztILb1ELb0ELi{fuse}ELb0EEvmmPKdliiiiiS1_S1_S1_S1_PdlS1_li"
            c, vops = count(kc[kn])
            f64 = sum(n for op, n in vops.items() if op.endswith("_f64"))
            m = meta[meta.index(".amdhsa_kernel " + kn):]
            res = [re.search(k + r"\s+(\d+)", m).group(1) for k in ("amdhsa_next_free_vgpr", "amdhsa_group_segment_fixed_size", "amdhsa_private_segment_fixed_size")]
            rep.append(f"  FUSE {fuse:3d} {what:44s} valu {c['valu']:5d} (f64 {f64:4d})  lds {c['lds']:3d}  vmem {c['vmem']:3d}  salu {c['salu']:4d}   VGPR {res[0]}, LDS {res[1]} B, scratch {res[2]} B")
        kp = kernel_bodies(os.path.join(d, "probe-hip-amdgcn-amd-amdhsa-gfx950.s"))
        e = count(kp["p_c_empty"])[0]["valu"]
        tw_own = count(kp["p_c_twiddles"])[0]["valu"] - count(kp["p_c_load1"])[0]["valu"]
        prod = count(kp["p_c_products"])[0]["valu"] - e
        full, out01 = count(kp["p_c_dft8_inv"])[0]["valu"] - e, count(kp["p_c_dft8_inv01"])[0]["valu"] - e
        rep.append("the pieces (compiled on their own, probe overhead subtracted), VALU per thread:")
        rep.append(f"  twiddle set w[2..7] from one loaded w[1] (pta_fft_twiddles<.., 1>: 6 complex products)   {tw_own:3d}   x 6 twiddled passes before")
        rep.append(f"  w[3], w[5], w[6], w[7] from tabulated w[1], w[2], w[4] (pta_fft_twiddle_products)          {prod:3d}   the two s = 64 passes with bit 32")
        rep.append(f"  8-point inverse butterfly pta_dft8<true>                                                {full:3d}")
        rep.append(f"  its outputs 0 and 1 only (pta_dft8_inv_out01)                                           {out01:3d}   the last pass with bit 64, window inside [0, 1024)")
        rep.append(f"removed per thread: bit 16 {tw_own} (last pass reuses the first pass's set), bit 32 {2 * tw_own} + {2 * (tw_own - prod)} (s = 8 sets complete from LDS, s = 64 sets four products "
                   f"from LDS), bit 64 {full - out01} + the post-chirp products and exec-masked store blocks of outputs 2..7; the table fill ({tw_own} + 8 in waves 0 and 1) and "
                   f"{2 * 7 + 2 * 3} ds_read_b128 per thread are added")
    path = os.path.join(ROOT, "profiles", "r17_isa_instruction_classes.txt")
    open(path, "w").write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main()
