"""The headline comparison against the parent commit: bench.py with default arguments in fresh processes, a build of the parent's
library (PTA_REPLICATOR_AMD_LIB) and this tree's library alternately, and before that one `--dump-outputs` run of each whose
residuals.npy must be the same file.

    python scripts/gpu_bench_alternate.py --parent-lib PATH [--runs 7] [--out FILE]

The bar (since round 13): parent median - new median >= 3 x (parent max - parent min), the parent's spread measured here.
A child that fails or runs out of its time limit ends the script: nothing more is started on the device."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(lib, extra=(), limit=180):
    env = dict(os.environ)
    env.pop("PTA_REPLICATOR_AMD_LIB", None)
    if lib:
        env["PTA_REPLICATOR_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *extra], env=env, capture_output=True, text=True,
                       timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        sys.exit(f"bench.py failed ({r.returncode}) with lib={lib}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_lib)
    res = {}
    with tempfile.TemporaryDirectory() as d:
        sums = {}
        for name, lib in (("parent", parent), ("new", None)):
            bench(lib, ["--steps", "2", "--warmup", "1", "--dump-outputs", os.path.join(d, name)])
            sums[name] = sha256(os.path.join(d, name, "residuals.npy"))
        res["residuals_sha256"] = sums
        res["residuals_identical"] = sums["parent"] == sums["new"]
    ms = {"parent": [], "new": []}
    for i in range(args.runs):
        for name, lib in (("parent", parent), ("new", None)):
            ms[name].append(round(bench(lib)["ms_per_step"], 4))
    spread = max(ms["parent"]) - min(ms["parent"])
    gain = statistics.median(ms["parent"]) - statistics.median(ms["new"])
    res.update({"ms_per_step": ms, "parent_median_ms": statistics.median(ms["parent"]), "new_median_ms": statistics.median(ms["new"]),
                "gain_ms": round(gain, 4), "parent_spread_ms": round(spread, 4), "bar_ms": round(3 * spread, 4), "bar_met": gain >= 3 * spread,
                "every_new_below_every_parent": max(ms["new"]) < min(ms["parent"])})
    txt = json.dumps(res, indent=1)
    if args.out:
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
