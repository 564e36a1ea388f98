"""The resampling behind SH-like branch supports (phyhip_calculate_sh_support, Statistics_To_SH on the device) at three pattern counts
on one device: P = 50 000 (cfg2), 10 000 (cfg3) and 100 000 (cfg5), siteCount = P, unit weights, 10 000 replicates, synthetic vectors
(a common base, independent noise per vector).  Per shape, in a process of its own under a time limit, the steps chained so that a
failure ends the run:
    whole call   host wall time of one call: table, totals, draws, count, the download of the two counts and the totals
    kernels      HIP events (phyhip_profile_read_support) around the four kernels
    fixed part   the same with ONE replicate: the table and totals kernels (the totals are a serial chain over the patterns) and
                 the launches; draws per second and gathered bytes per second (64 bytes per draw) follow from kernels - fixed part
Median of --reps after --warm warm ones.  The host side of the comparison is the REFERENCE's own Statistics_To_SH, timed per internal
edge by tests/golden/make_sh.py on the machine that generated tests/golden/sh_support_*.npz (one host thread, 886 / 547 sites):
another machine than the device's host, so the ratio is an order of magnitude, not a measurement of one system.
    python tools/sh_support_timing.py [--out profiles/sh_support.md] [--reps 3] [--warm 1]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SHAPES = [(50000, 240), (10000, 240), (100000, 300)]   # (patterns = sites, seconds allowed)
REPLICATES = 10000


def one(P, warm, reps):
    from phyml_amd import capi
    rng = np.random.default_rng(P)
    base = -2.0 - 6.0 * rng.random(P)
    lks = base[None, :] + 0.3 * (rng.random((3, P)) - 0.5)
    inst = capi.Instance(4, 10, 4, P, 5, 1, device=0)
    try:
        inst.set_pattern_weights(np.ones(P))
        for k in range(3):
            inst.set_support_site_lnl(k, lks[k])
        inst.profile(1)
        wall, kms, res = [], [], None
        for r in range(warm + reps):
            inst.profile_read_support()
            t0 = time.perf_counter()
            got = inst.sh_support(P, REPLICATES, 12345)
            dt = time.perf_counter() - t0
            ms, calls = inst.profile_read_support()
            assert calls == 1 and (res is None or got[:2] == res[:2])
            res = got
            if r >= warm:
                wall.append(dt); kms.append(ms)
        fixed = []
        for r in range(warm + reps):
            inst.profile_read_support()
            inst.sh_support(P, 1, 12345)
            ms, calls = inst.profile_read_support()
            if r >= warm:
                fixed.append(ms)
        inst.profile(0)
        k0 = float(np.median(fixed))
        k = float(np.median(kms)) - k0
        assert k > 0
        draws = float(REPLICATES) * P
        return dict(patterns=P, sites=P, replicates=REPLICATES, ms_call=float(np.median(wall)) * 1e3, ms_kernels=float(np.median(kms)), ms_fixed=k0, draws=draws,
                    draws_per_s=draws / (k * 1e-3), gather_bytes_per_s=64.0 * draws / (k * 1e-3), table_bytes=64 * P, sh=res[0], rell=res[1])
    finally:
        inst.close()


def host_reference():
    """[(fixture, sites, median seconds per Statistics_To_SH, ns per draw)] from the committed golden files"""
    out = []
    for name in ("nucleic", "proteic"):
        fx = np.load(os.path.join(ROOT, "tests", "golden", "sh_support_" + name + ".npz"))
        s, sites = float(np.median(fx["seconds"][:, 0])), int(fx["init_len"][0])
        out.append((name, sites, s, s / (REPLICATES * sites) * 1e9))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sh_support.md"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shape", type=int)
    a = ap.parse_args()
    if a.shape:   # one step, in this process
        print("SHSUPPORT " + json.dumps(one(a.shape, a.warm, a.reps)))
        return
    rows = []
    for P, limit in SHAPES:   # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(P), "--reps", str(a.reps), "--warm", str(a.warm)],
                               timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"P = {P} ran out of its {limit} s")
        if r.returncode != 0:
            raise SystemExit(f"P = {P} failed with status {r.returncode}")
        rows.append(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("SHSUPPORT "))[len("SHSUPPORT "):]))
        print(json.dumps(rows[-1]), flush=True)
    host = host_reference()
    ns = float(np.mean([h[3] for h in host]))
    with open(a.out, "w") as f:
        f.write("| patterns = sites | draws | whole call ms | kernels ms | of which with one replicate ms | draws / s | gathered bytes / s (64 B per draw) | table | "
                "reference on one host thread, extrapolated at %.0f ns per draw |\n|---|---|---|---|---|---|---|---|---|\n" % ns)
        for r in rows:
            f.write("| %d | %.1e | %.1f | %.1f | %.2f | %.2e | %.2e | %.1f MB | %.0f s |\n" % (
                r["patterns"], r["draws"], r["ms_call"], r["ms_kernels"], r["ms_fixed"], r["draws_per_s"], r["gather_bytes_per_s"], r["table_bytes"] / 1e6,
                r["draws"] * ns * 1e-9))
        f.write("\nThe reference's own Statistics_To_SH, per internal edge, as timed where the golden files were generated: "
                + "; ".join("%s (%d sites) %.2f s = %.0f ns per draw" % h for h in host) + ".\n")


if __name__ == "__main__":
    main()
