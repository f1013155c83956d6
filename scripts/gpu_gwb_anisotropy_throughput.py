"""Throughput of the anisotropic GWB per realisation (theta key gwb_clm) against the power-law theta path of the same engine, headline
configuration (68 pulsars x 5000 TOAs, GWB + RN + EFAC/EQUAD + ECORR) with set_gwb(lmax=L), L = 1 and 4, R realisations per batch,
timed with HIP events in ONE process:

  power_law_l<L>   eng_L.generate(R, theta={gwb_log10_A, gwb_gamma})
  clm_l<L>         eng_L.generate(R, theta={gwb_clm [R, (L+1)^2], gwb_log10_A, gwb_gamma})

The modes alternate step by step after a warm-up, so clock drift hits all alike.  The two new kernels are also timed on their own
beside what they replace, on the same shapes: pta_gwb_mix_batched / pta_gwb_mix (the same HBM bytes), and pta_gwb_orf_factor / the
composition of existing pieces for the same R factors (pta_dgemm for clm . basis + pta_potrf_batched_ex with forward-substitution
panel solves and the zeroed upper triangle).  Prints one JSON line; --out also writes it to a file.

    timeout -k 10 300 python scripts/gpu_gwb_anisotropy_throughput.py --steps 20 --warmup 3 --out profiles/r19_gwb_anisotropy_throughput.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import configure_engine, headline_array  # noqa: E402
from pta_replicator_amd import _hyper, _lib, device as dv  # noqa: E402
from pta_replicator_amd.engine import ReplicaEngine  # noqa: E402


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stats(t):
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="launches per per-kernel timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    psrs, noise = headline_array(68, 5000)
    rng = np.random.default_rng(1)
    c00 = np.sqrt(4.0 * np.pi)
    engs, thetas = {}, {}
    pl_theta = {"gwb_log10_A": torch.as_tensor(rng.uniform(-15, -14, R), device="cuda"), "gwb_gamma": torch.as_tensor(rng.uniform(3, 5, R), device="cuda")}
    for L in (1, 4):
        n = (L + 1) ** 2
        eng = configure_engine(ReplicaEngine(psrs, seed=1234), noise)
        eng.set_gwb(noise["gw_log10_A"], 13. / 3., clm=[c00] + [0.0] * (n - 1), lmax=L)
        engs[L] = eng.prepare()
        # |c_lm| <= 0.5 / sqrt(n - 1): the power stays positive, every ORF positive definite
        clm = np.concatenate([np.full((R, 1), c00), rng.uniform(-0.5, 0.5, (R, n - 1)) / np.sqrt(n - 1)], axis=1)
        thetas[L] = dict(pl_theta, **{_hyper.CLM_KEY: torch.as_tensor(clm, device="cuda")})
    out = dv.empty((R, engs[1].n_toa))
    state = {"r0": 0}
    runs = {}
    for L in (1, 4):
        runs[f"power_law_l{L}"] = lambda L=L: engs[L].generate(R, r0=state["r0"], out=out, theta=pl_theta)
        runs[f"clm_l{L}"] = lambda L=L: engs[L].generate(R, r0=state["r0"], out=out, theta=thetas[L])
    for _ in range(a.warmup):
        for f in runs.values():
            f()
        state["r0"] += R
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.steps):
        for k, f in runs.items():
            times[k].append(event_ms(f))
        state["r0"] += R

    # the new kernels on their own, beside what they replace (same batch, same workspace)
    s = dv.stream_ptr()
    P = engs[1].P
    kern = {}
    ws = engs[4]._ws
    npts = engs[4].plan.gw_npts
    mix = (P, dv.ptr(ws["G0"]), R, npts, npts, dv.ptr(ws["G"]), 0, s)
    kern["gwb_mix_ms"] = lambda: _lib.call("pta_gwb_mix", dv.ptr(engs[4].d_M), *mix)
    kern["gwb_mix_batched_ms"] = lambda: _lib.call("pta_gwb_mix_batched", dv.ptr(ws["mchol"]), P * P, *mix)
    info = dv.zeros((R,), dtype=torch.int32)
    for L in (1, 4):
        eng, n = engs[L], (L + 1) ** 2
        clm, basis, M = thetas[L][_hyper.CLM_KEY], engs[L].d_orf_basis, engs[L]._ws["mchol"]
        kern[f"gwb_orf_factor_l{L}_ms"] = (lambda clm=clm, basis=basis, M=M, n=n: _lib.call(
            "pta_gwb_orf_factor", dv.ptr(basis), n, P, dv.ptr(clm), n, R, dv.ptr(M), dv.ptr(info), s))

        def composed(clm=clm, basis=basis, M=M, n=n):
            _lib.call("pta_dgemm", 0, R, P * P, n, 2.0, dv.ptr(clm), n, 1, dv.ptr(basis), P * P, 0.0, dv.ptr(M), P * P,
                      0, 1, 0, 0, 0, 1, s)
            _lib.call("pta_potrf_batched_ex", dv.ptr(M), P, P, P * P, R, dv.ptr(info), _lib.POTRF_SUBSTITUTION | _lib.POTRF_ZERO_UPPER, s)
        kern[f"dgemm_potrf_l{L}_ms"] = composed
    kernels = {}
    for name, fn in kern.items():
        fn()
        kernels[name] = stats([event_ms(fn, a.reps) for _ in range(5)])
    torch.cuda.synchronize()
    assert not info.any()

    med = {k: float(np.median(t)) for k, t in times.items()}
    res = dict(
        config="68 x 5000, GWB (set_gwb(lmax=L), L = 1 / 4) + RN(67) + EFAC/EQUAD + ECORR, throughput mode, czt transform",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, npts=npts,
        generate_ms={k: stats(t) for k, t in times.items()},
        realisations_per_s={k: round(R / v * 1e3, 1) for k, v in med.items()},
        clm_over_power_law={f"l{L}": round(med[f"clm_l{L}"] / med[f"power_law_l{L}"], 4) for L in (1, 4)},
        mix_bytes=16 * R * P * npts,
        kernels_ms=kernels,
    )
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
