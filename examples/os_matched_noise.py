"""The optimal statistic over a prior on the noise parameters: every realisation has its own red noise, drawn on the GPU from
rn_log10_A ~ U(-15, -12.5), rn_gamma ~ U(2, 6) per pulsar.  No GWB is injected, so the SNR of a calibrated statistic has zero mean and
unit variance.

  fixed     generate_os(R, theta=theta)                 every realisation weighted with the one configured noise model
  matched   generate_os(R, theta=theta, matched=True)   every realisation weighted with the noise model it was generated with

    python examples/os_matched_noise.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import configure_engine, headline_array                      # synthetic array with the NANOGrav 15-yr noise dictionary's shape
from pta_replicator_amd.engine import ReplicaEngine

P, N, R = 24, 2000, 4096
psrs, noise = headline_array(P, N)
eng = configure_engine(ReplicaEngine(psrs, seed=21), noise)
eng._gw = None                                                         # no GWB in the injection
eng.set_hyper_prior(rn_log10_A=(-15.0, -12.5), rn_gamma=(2.0, 6.0))
eng.prepare()
eng.prepare_optimal_statistic(components=14, gwb_auto=False, matched=True)
theta = eng.sample_theta(R)                                            # what generate_sampled(R) would draw: a pure function of (seed, r)
fixed = eng.generate_os(R, theta=theta)
matched = eng.generate_os(R, theta=theta, matched=True)
print(f"{P} pulsars x {N} TOAs, {R} realisations, red noise ~ prior, no GWB; ORFs {matched['names']}")
for name, res in (("fixed-noise", fixed), ("matched", matched)):
    snr = res["snr"].cpu().numpy()
    print(f"  {name:12s} null SNR mean {snr.mean(0).round(3)}  std {snr.std(0).round(3)}")
print("sigma of the matched statistic is per realisation:", tuple(matched["sigma"].shape), "against", tuple(fixed["sigma"].shape))
