"""The pairwise ML distance matrix (phyhip_calculate_pairwise_ml_distances, ML_Dist on the device) at three shapes on one device:
100 x 50 000 nt (cfg2), 200 x 10 000 aa (cfg3) and 500 x 100 000 nt (cfg5).  Per shape, in a process of its own under a time limit,
the steps chained so that a failure ends the run:
    whole call       host wall time of one call, the starting values' round trip and the download of the matrix included
    count kernels    HIP events (phyhip_profile_read_pairwise): dist_count_kernel + the per-pair sums, also as the share of the FP64
                     matrix peak its issued v_mfma_f64_16x16x4_f64 reach (2048 FLOP each; 78.6 TFLOP/s, the data sheet's figure)
    optimiser        HIP events around dist_opt_kernel
Median of --reps after --warm warm ones.  The host baseline (last step, smallest shape only): the wall-clock difference between
oracle/_ref/phyml_ref_driver dump --model-only run without -u (ML_Dist + BioNJ) and with -u (a given tree) on the same alignment
-- a difference of two wall times that includes BioNJ: one digit.
    python tools/pairwise_timing.py [--out profiles/pairwise_distances.md] [--reps 3] [--warm 1] [--no-baseline]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SHAPES = [("cfg2_nt_100x50k", 240), ("cfg3_aa_200x10k", 240), ("cfg5_nt_500x100k", 420)]   # (workload, seconds allowed)
FP64_MATRIX_FLOPS = 78.6e12
DRIVER = os.path.join(ROOT, "oracle", "_ref", "phyml_ref_driver")


def issued_mfma(n, S, P):
    """v_mfma_f64_16x16x4_f64 instructions dist_count_kernel issues for one band holding every taxon (phyhip_dist.hip)"""
    ldg = (n * S + 63) // 64 * 64
    row_blocks = ((n - 1) * S + 15) // 16
    live = 0
    for rb in range(row_blocks):
        row_min_taxon = (16 * rb) // S
        for ct in range(ldg // 16):
            live += (16 * ct + 15) // S > row_min_taxon
    return live * ((P + 15) // 16) * 4


def one(name, warm, reps):
    from phyml_amd import capi, workloads
    wl = workloads.make(name)
    st, blk, cfg = wl["states"], wl["model"], wl["cfg"]
    n, P, S = st.shape[0], st.shape[1], cfg["ns"]
    inst = capi.Instance(n, 2 * n, S, P, 2 * n, 1, device=0)
    try:
        inst.set_pattern_weights(np.ones(P))
        inst.set_category_rates([1.0]); inst.set_category_weights([1.0])
        inst.set_state_frequencies(blk["pi"])
        inst.set_eigen_decomposition(blk["r_e_vect"], blk["l_e_vect"], blk["e_val"])
        inst.set_phyml_options(float(blk["l_min"][0]), float(blk["l_max"][0]), 1.0, 1)
        for t in range(n):
            inst.set_tip_states(t, st[t].astype(np.int32))
        inst.profile(1)
        wall, cms, oms = [], [], []
        for r in range(warm + reps):
            inst.profile_read_pairwise()
            t0 = time.perf_counter()
            D, extra = inst.pairwise_ml_distances(1e-3, want=("iterations",))
            dt = time.perf_counter() - t0
            a, b, calls = inst.profile_read_pairwise()
            assert calls == 1
            if r >= warm:
                wall.append(dt); cms.append(a); oms.append(b)
        inst.profile(0)
        mf = issued_mfma(n, S, P)
        ms_count = float(np.median(cms))
        return dict(workload=name, taxa=n, patterns=P, states=S, pairs=n * (n - 1) // 2, ms_call=float(np.median(wall)) * 1e3, ms_count=ms_count,
                    ms_optimise=float(np.median(oms)), mfma_issued=mf, mfma_share_of_fp64_peak=mf * 2048 / (ms_count * 1e-3) / FP64_MATRIX_FLOPS,
                    iterations_min=int(extra["iterations"].min()), iterations_max=int(extra["iterations"].max()),
                    max_distance=float(D.max()), mean_distance=float(D[np.triu_indices(n, 1)].mean()))
    finally:
        inst.close()


def host_baseline(name, limit):
    """seconds(reference run without -u) - seconds(with -u), or None where the reference driver was not built"""
    if not os.path.exists(DRIVER):
        return None
    from phyml_amd import synth, workloads
    wl = workloads.make(name)
    tree, st, cfg = wl["tree"], wl["states"], wl["cfg"]
    tmp = tempfile.mkdtemp(prefix="pairwise_")
    ali, tre = os.path.join(tmp, "a.phy"), os.path.join(tmp, "t.nwk")
    synth.write_phylip(ali, tree.names, synth.states_to_chars(st, cfg["ns"]))
    open(tre, "w").write(tree.to_newick() + "\n")
    margs = ["-d", "nt", "-m", "GTR", "-f", "0.3,0.2,0.2,0.3"] if cfg["ns"] == 4 else ["-d", "aa", "-m", "LG", "-f", "m"]
    tail = margs + ["-c", "4", "-a", "1.0", "-o", "n", "-b", "0"]
    secs = []
    for extra in ([], ["-u", tre]):
        t0 = time.perf_counter()
        subprocess.run([DRIVER, "dump", os.path.join(tmp, "m.phyg"), "--model-only", "--", "-i", ali] + extra + tail, check=True, timeout=limit,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        secs.append(time.perf_counter() - t0)
    return secs[0] - secs[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_distances.md"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--shape")
    ap.add_argument("--baseline-of")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    if a.shape:   # one step, in this process
        print("PAIRWISE " + json.dumps(one(a.shape, a.warm, a.reps)))
        return
    if a.baseline_of:
        print("PAIRWISE " + json.dumps(dict(host_seconds=host_baseline(a.baseline_of, 380))))
        return
    rows = []
    steps = [(["--shape", name, "--reps", str(a.reps), "--warm", str(a.warm)], limit) for name, limit in SHAPES]
    if not a.no_baseline:
        steps.append((["--baseline-of", SHAPES[0][0]], 800))
    for args, limit in steps:   # (a step that fails or runs out of time ends the run: nothing more is started on the device)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            if args[0] != "--baseline-of":
                raise SystemExit(f"step {args} ran out of its {limit} s")
            r = subprocess.CompletedProcess(args, 124, "")
        if r.returncode != 0 and args[0] == "--baseline-of":   # (host only, and the last step: the device figures are still written)
            rows.append(dict(host_seconds=None))
            continue
        if r.returncode != 0:
            raise SystemExit(f"step {args} failed with status {r.returncode}")
        rows.append(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("PAIRWISE "))[len("PAIRWISE "):]))
        print(json.dumps(rows[-1]), flush=True)
    base = rows.pop()["host_seconds"] if not a.no_baseline else None
    with open(a.out, "w") as f:
        f.write("# Pairwise ML distances (ML_Dist) on the device\n\n"
                "`tools/pairwise_timing.py` on one MI355X, one process per shape; medians of %d calls after %d warm-up(s); integer weights, "
                "`min_diff_lk_local` = 1e-3, starting values from the device's counts (the host round trip is inside the whole call).\n\n"
                "| workload | pairs | whole call ms | count kernels ms | optimiser ms | MFMA issued | share of the FP64 matrix peak (78.6 TFLOP/s) | Brent iterations |\n"
                "|---|---|---|---|---|---|---|---|\n" % (a.reps, a.warm))
        for r in rows:
            f.write("| %s (%d x %d patterns x %d states) | %d | %.1f | %.2f | %.2f | %.3g | %.1f %% | %d..%d |\n" % (
                r["workload"], r["taxa"], r["patterns"], r["states"], r["pairs"], r["ms_call"], r["ms_count"], r["ms_optimise"], r["mfma_issued"],
                100.0 * r["mfma_share_of_fp64_peak"], r["iterations_min"], r["iterations_max"]))
        if not a.no_baseline and base is None:
            f.write("\nHost baseline at %s: not measured (the reference driver is not built here, or a run exceeded its time limit).\n" % SHAPES[0][0])
        if base is not None:
            f.write("\nHost baseline at %s: the reference run without `-u` took about %.0e s longer than with `-u` (`phyml_ref_driver dump "
                    "--model-only`; ML_Dist + BioNJ on one host core, a difference of two wall times: one digit).\n" % (SHAPES[0][0], base))
        f.write("\n20 states run the same 16 x 16 x 4 instruction on the flattened (taxon, state) index, so no lane is padding; the 16 + 4 "
                "packing and the 32-row padding of the state axis were not built.\n")


if __name__ == "__main__":
    main()
