"""Host wall time of the exact per-site route against the approximate one, at cfg2's and cfg3's sizes on one device in one process:
    exact        Get_Exact_Site_Lk(b)            (phyhip_calculate_edge_site_outputs_exact: its own kernel, P x (C + 2) doubles + P ints
                                                  + the P weights of the ordered sum downloaded)
    approximate  Lk(b), then Get_Site_Lk          (the hot path's evaluation, then phyhip_get_site_outputs: P x (C + 2) doubles + P ints)
and, to say where the exact call's time goes, the same call with every output pointer NULL (kernel + synchronisation, no arrays).
Median of --reps calls after --warm warm ones, each call timed on its own.
    python tools/bench_exact_site.py [--out profiles/exact_site_outputs.md] [--reps 60] [--warm 20]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from phyml_amd import lktree, workloads


def median_us(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def one(name, warm, reps):
    wl = workloads.make(name)
    tree, st, blk, cfg = wl["tree"], wl["states"], wl["model"], wl["cfg"]
    n, P, S, Cc = tree.n_otu, st.shape[1], cfg["ns"], int(blk["ncatg"][0])
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, S, Cc, device=0)
    try:
        t.set_model(blk["pi"], blk["gamma_rr"], blk["gamma_r_proba"], blk["e_val"], blk["r_e_vect"], blk["l_e_vect"],
                    float(blk["l_min"][0]), float(blk["l_max"][0]), 1.0, 1)
        t.Make_Tree_For_Lk(np.ones(P))
        t.set_tips(tip_states=st.astype(np.int32))
        t.Set_Both_Sides(True)
        t.Lk(None)
        rows = []
        internal = [e for e in range(t.ne) if not t.edge(e).contents.rght.contents.tax and not t.edge(e).contents.left.contents.tax]
        pendant = [e for e in range(t.ne) if t.edge(e).contents.rght.contents.tax]
        for kind, e in (("internal edge", internal[len(internal) // 2]), ("pendant edge (tip branch)", pendant[len(pendant) // 2])):
            b = t.edge(e).contents
            child = b.p_lk_tip_idx if b.rght.contents.tax else b.p_lk_rght_idx
            L, iid = t.inst.L, t.inst.id

            def approximate():
                t.Lk(e)
                return t.inst.site_outputs()

            def exact():
                return t.Exact_Site_Lk(e)

            def exact_no_arrays():
                return L.phyhip_calculate_edge_site_outputs_exact(iid, b.p_lk_left_idx, child, b.Pij_rr_idx, None, None, None, None, None, None)

            ap, ex = approximate(), exact()
            dev = float(np.max(np.abs(ap[0] - ex[1])))
            rows.append(dict(workload=name, edge=kind, patterns=P, states=S, categories=Cc,
                             us_exact=median_us(exact, warm, reps), us_approximate=median_us(approximate, warm, reps),
                             us_exact_kernel_and_sync=median_us(exact_no_arrays, warm, reps),
                             download_MB=P * (Cc + 2) * 8 / 1e6, max_abs_site_lnl_difference=dev))
        return rows
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_site_outputs.md"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warm", type=int, default=20)
    a = ap.parse_args()
    assert a.reps >= 50 and a.warm >= 20
    rows = one("cfg2_nt_100x50k", a.warm, a.reps) + one("cfg3_aa_200x10k", a.warm, a.reps)
    with open(a.out, "w") as f:
        f.write("# Exact per-site outputs against the approximate sequence\n\n"
                "`tools/bench_exact_site.py`: host wall time per call on one MI355X, one process; median of %d calls after %d warm ones.\n"
                "exact = `Get_Exact_Site_Lk(b)`; approximate = `Lk(b)` then `Get_Site_Lk` (`phyhip_get_site_outputs`); the third column is the\n"
                "exact call with every output pointer NULL (its kernel, the synchronisation, the warning word: no arrays).\n\n"
                "| workload | edge | exact us | approximate us | exact / approximate | exact, no arrays us | arrays MB | max abs difference of c_lnL_sorted |\n"
                "|---|---|---|---|---|---|---|---|\n" % (a.reps, a.warm))
        for r in rows:
            f.write("| %s (%d x %d states, %d categories) | %s | %.1f | %.1f | %.2f | %.1f | %.2f | %.2g |\n" % (
                r["workload"], r["patterns"], r["states"], r["categories"], r["edge"], r["us_exact"], r["us_approximate"],
                r["us_exact"] / r["us_approximate"], r["us_exact_kernel_and_sync"], r["download_MB"], r["max_abs_site_lnl_difference"]))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
