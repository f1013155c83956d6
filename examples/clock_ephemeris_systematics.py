"""Clock and ephemeris systematics beside a Hellings-Downs background: what the HD statistics say when a monopole (a clock error)
and a dipole (a Solar-system ephemeris error) are in the data, and what the foils say.

    python examples/clock_ephemeris_systematics.py

Two engines on the same array and seed: an HD background alone, and the same background plus a monopole and a dipole process
(add_common_process).  Every deviate is a function of (seed, realisation, stream), so the second engine's rows are the first engine's
plus the two processes, element by element.  For both, the optimal-statistic SNR of the three ORFs and the likelihood ratio ln B of
four ORFs against noise alone, at the injected amplitude.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pta_replicator_amd.engine import ReplicaEngine
from pta_replicator_amd.simulate import ArrayTOAs, SimulatedPulsar, make_ideal

P, N, R, NF = 20, 400, 512, 5
GW_A, GAMMA = -14.3, 13. / 3.
rng = np.random.default_rng(7)
psrs = []
for a in range(P):
    psr = SimulatedPulsar(toas=ArrayTOAs(np.sort(rng.uniform(53000, 58000, N)), 0.2), name=f"J{a:04d}",
                          loc={"RAJ": float(rng.uniform(0, 24)), "DECJ": float(np.degrees(np.arcsin(rng.uniform(-1, 1))))})
    make_ideal(psr)
    psrs.append(psr)


def engine(systematics):
    eng = ReplicaEngine(psrs, seed=2026)
    eng.set_white_noise(efac=1.0)
    eng.set_gwb(GW_A, GAMMA)
    if systematics:
        eng.add_common_process(-14.1, 3.0, orf="monopole", components=NF)    # a clock error: the same delay in every pulsar
        eng.add_common_process(-14.0, 2.5, orf="dipole", components=NF)      # an ephemeris error: cos(angle) between pulsars
    return eng.prepare()


clean, dirty = engine(False), engine(True)
print("configured:", dirty.common_processes)
sig = dirty.generate_per_signal(4)
print("RMS [us] of the GWB %.3f and of the two systematics together %.3f; rows = clean rows + that term: %s"
      % (1e6 * float(sig["gwb"].std()), 1e6 * float(sig["common"].std()), bool((dirty.generate(4) == clean.generate(4) + sig["common"]).all())))

orfs = ("hd", "monopole", "dipole")
for name, eng in (("HD background alone", clean), ("+ clock and ephemeris errors", dirty)):
    # the fixed-noise statistics of an engine weight with the noise it generates: the auto-terms of the processes are in C_a
    eng.prepare_optimal_statistic(components=NF, orfs=orfs)
    snr = eng.generate_os(R)["snr"].cpu().numpy().mean(axis=0)
    eng.prepare_correlated_likelihood(components=NF, orfs=orfs + ("curn",))
    lam = eng.generate_correlated_lnl(R, {"gwb_log10_A": np.array([GW_A])})["lnl_ratio"][:, :, 0].cpu().numpy().mean(axis=0)
    print("%-30s mean OS SNR  " % name + "  ".join("%s %+6.2f" % (o, v) for o, v in zip(orfs, snr)))
    print("%-30s mean ln B    " % "" + "  ".join("%s %+7.2f" % (o, v) for o, v in zip(orfs + ("curn",), lam)))

# amplitudes per realisation: theta's cp_log10_A / cp_gamma [R, n_proc], or drawn on chip from uniform boxes with the labels returned
dirty.set_hyper_prior(cp_log10_A=[[-15.0, -13.8], [-15.0, -13.8]], cp_gamma=(1.0, 5.0))
rows, theta = dirty.generate_sampled(256)
print({k: tuple(v.shape) for k, v in theta.items()})
