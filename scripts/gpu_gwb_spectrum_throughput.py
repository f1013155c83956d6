"""Throughput of the per-realisation GWB spectrum (theta key gwb_log10_hc) against the fixed userSpec engine and against the
power-law theta path, headline configuration (68 pulsars x 5000 TOAs, HD GWB + RN + EFAC/EQUAD + ECORR), R realisations per batch,
timed with HIP events in ONE process:

  fixed_userspec   eng_u.generate(R)                                        (userSpec engine, M = 14 nodes)
  spec_M14         eng_u.generate(R, theta={gwb_log10_hc [R, 14]})
  spec_M64         eng_v.generate(R, theta={gwb_log10_hc [R, 64]})          (userSpec engine, M = 64 nodes)
  power_law        eng_p.generate(R, theta={gwb_log10_A, gwb_gamma})        (power-law engine: the yardstick)

The modes alternate step by step after a warm-up, so clock drift hits all alike.  The new kernels are also timed on their own beside
their power-law counterparts: pta_gwb_spectrum_scale_user / pta_gwb_spectrum_scale and pta_os_matched_prior_spec /
pta_os_matched_prior.  Prints one JSON line; --out also writes it to a file.

    timeout -k 10 300 python scripts/gpu_gwb_spectrum_throughput.py --steps 20 --warmup 3 --out profiles/r15_gwb_spectrum_throughput.json
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


def user_spec(M, log10_A):
    """M nodes over 1e-9 .. 3e-7 Hz on the gamma = 13/3 power law of the headline amplitude"""
    f = 10 ** np.linspace(-9, np.log10(3e-7), M)
    return np.stack([f, 10 ** (log10_A - (2. / 3.) * np.log10(f * 3.16e7))], axis=1)


def stats(t):
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="launches per per-kernel timing")
    ap.add_argument("--components", type=int, default=14)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    R = a.batch
    psrs, noise = headline_array(68, 5000)
    rng = np.random.default_rng(1)
    eng_p = configure_engine(ReplicaEngine(psrs, seed=1234), noise).prepare()
    engs, specs = {}, {}
    for M in (14, 64):
        U = user_spec(M, noise["gw_log10_A"])
        eng = configure_engine(ReplicaEngine(psrs, seed=1234), noise)
        eng.set_gwb(noise["gw_log10_A"], 13. / 3., userSpec=U)
        engs[M] = eng.prepare()
        specs[M] = {_hyper.SPEC_KEY: torch.as_tensor(np.log10(U[:, 1])[None, :] + rng.uniform(-0.5, 0.5, (R, M)), device="cuda")}
    pl_theta = {"gwb_log10_A": torch.as_tensor(rng.uniform(-15, -14, R), device="cuda"), "gwb_gamma": torch.as_tensor(rng.uniform(3, 5, R), device="cuda")}
    out = dv.empty((R, eng_p.n_toa))
    state = {"r0": 0}
    runs = {
        "fixed_userspec": lambda: engs[14].generate(R, r0=state["r0"], out=out),
        "spec_M14": lambda: engs[14].generate(R, r0=state["r0"], out=out, theta=specs[14]),
        "spec_M64": lambda: engs[64].generate(R, r0=state["r0"], out=out, theta=specs[64]),
        "power_law": lambda: eng_p.generate(R, r0=state["r0"], out=out, theta=pl_theta),
    }
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

    # the new kernels on their own, beside their power-law counterparts (same batch, same workspace rows)
    s = dv.stream_ptr()
    kern = {}
    hp, wp, gw = eng_p._hyper_tables(), eng_p._ws, eng_p._gw
    Nf = eng_p.grid["Nf"]
    kern["gwb_spectrum_scale_ms"] = lambda: _lib.call(
        "pta_gwb_spectrum_scale", dv.ptr(hp["gw_f"]), dv.ptr(hp["gw_hcf0"]), Nf, R, dv.ptr(pl_theta["gwb_log10_A"]), dv.ptr(pl_theta["gwb_gamma"]),
        int(bool(gw["turnover"])), float(gw["f0"]), float(gw["beta"]), float(gw["power"]), dv.ptr(wp["scale"]), Nf, s)
    for M in (14, 64):
        hy, ws, y = engs[M]._hyper_tables(), engs[M]._ws, specs[M][_hyper.SPEC_KEY]
        kern[f"gwb_spectrum_scale_user_M{M}_ms"] = (lambda hy=hy, ws=ws, y=y, M=M: _lib.call(
            "pta_gwb_spectrum_scale_user", dv.ptr(hy["spec_seg"]), dv.ptr(hy["spec_dx"]), dv.ptr(hy["spec_dxp"]), dv.ptr(hy["gw_hcf0"]), Nf, M, R,
            dv.ptr(y), M, dv.ptr(ws["scale"]), Nf, s))
    # the prior kernels of the matched statistic (same array, same theta rows)
    eng_p.prepare_optimal_statistic(components=a.components, matched=True)
    m = eng_p._os["matched"]
    P, C, K_rn = eng_p.P, eng_p._os["C"], m["K_rn"]
    b = dv.empty((R, P * m["K"]))
    rn_lA = torch.as_tensor(rng.uniform(-15, -13, (R, P)), device="cuda")
    rn_g = torch.as_tensor(rng.uniform(2, 6, (R, P)), device="cuda")
    rn_args = (dv.ptr(hp["rn_f"]), dv.ptr(hp["rn_tspan"]), dv.ptr(m["rn_phi"]), dv.ptr(rn_lA), dv.ptr(rn_g), m["T"])
    kern["os_matched_prior_ms"] = lambda: _lib.call("pta_os_matched_prior", R, P, K_rn, C, *rn_args, dv.ptr(pl_theta["gwb_log10_A"]),
                                                    dv.ptr(pl_theta["gwb_gamma"]), dv.ptr(m["s"]), dv.ptr(b), s)
    fk = np.arange(1, C // 2 + 1) / m["T"]
    for M in (14, 64):
        _, xp = _hyper.spec_nodes(engs[M]._gw["userSpec"])
        seg, dx, dxp = _hyper.spec_tables(fk, xp)
        tab = (dv.i32(seg), dv.f64(dx), dv.f64(dxp))
        y = specs[M][_hyper.SPEC_KEY]
        kern[f"os_matched_prior_spec_M{M}_ms"] = (lambda tab=tab, y=y, M=M: _lib.call(
            "pta_os_matched_prior_spec", R, P, K_rn, C, *rn_args, dv.ptr(tab[0]), dv.ptr(tab[1]), dv.ptr(tab[2]), M, dv.ptr(y), M, dv.ptr(m["s"]),
            dv.ptr(b), s))
    kernels = {}
    for name, fn in kern.items():
        fn()
        kernels[name] = stats([event_ms(fn, a.reps) for _ in range(5)])
    torch.cuda.synchronize()

    med = {k: float(np.median(t)) for k, t in times.items()}
    res = dict(
        config="68 x 5000, HD GWB + RN(67) + EFAC/EQUAD + ECORR, throughput mode, czt transform; userSpec engines with M = 14 / 64 nodes",
        device=torch.cuda.get_device_name(0), batch=R, steps=a.steps, warmup=a.warmup, Nf=Nf, os_components=a.components,
        generate_ms={k: stats(t) for k, t in times.items()},
        realisations_per_s={k: round(R / v * 1e3, 1) for k, v in med.items()},
        spec_M14_over_power_law=round(med["spec_M14"] / med["power_law"], 4), spec_M64_over_power_law=round(med["spec_M64"] / med["power_law"], 4),
        spec_M14_over_fixed_userspec=round(med["spec_M14"] / med["fixed_userspec"], 4),
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
