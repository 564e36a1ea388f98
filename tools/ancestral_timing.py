"""Marginal ancestral state posteriors: the device route against the download route it replaces, at cfg2's and cfg3's shapes on one
device in one process, after Set_Both_Sides(YES); Lk(NULL):
    (a) the new call      Get_All_Ancestral_Probs: phyhip_calculate_node_state_posteriors for all n - 2 internal nodes in one call,
                          the download of the (n - 2) x P x S doubles included (host wall time)
    (b) its kernel alone  HIP events around the launch (phyhip_profile_read_node_posteriors), also as algorithmic bytes / time against
                          8 TB/s: per (node, pattern) three side reads (C x S doubles, or one tip byte), three scale reads (4 bytes
                          per non-tip side) and one result write (S doubles)
    (c) the old route     INTEGRATION.md's `--ancestral` paragraph: phyhip_get_partials + phyhip_get_scale_factors for all 3(n - 2)
                          internal side buffers -- the downloads only, no host arithmetic: a LOWER bound of the route
Median of --reps after --warm warm ones, each timed on its own.
    python tools/ancestral_timing.py [--out profiles/ancestral_posteriors.md] [--reps 20] [--warm 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from phyml_amd import lktree, workloads

HBM_BYTES_PER_S = 8e12


def medians(fn, warm, reps):
    """(median wall seconds, median of what fn returns) over reps calls after warm ones"""
    for _ in range(warm):
        fn()
    ts, vs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        v = fn()
        ts.append(time.perf_counter() - t0)
        vs.append(0.0 if v is None else v)
    return float(np.median(ts)), float(np.median(vs))


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
        # the internal side buffers of the tree: 3 per internal node, 3(n - 2) in all
        bufs, tip_sides = [], 0
        for e in range(t.ne):
            b = t.edge(e).contents
            for node, idx in ((b.left.contents, b.p_lk_left_idx), (b.rght.contents, b.p_lk_rght_idx)):
                if node.tax:
                    tip_sides += 1
                else:
                    bufs.append(idx)
        assert len(bufs) == 3 * (n - 2) and tip_sides == n
        out = np.zeros((n - 2, P, S))
        part = np.zeros((P, Cc * S))
        scal = np.zeros(P, np.int32)
        L, iid = t.inst.L, t.inst.id
        dp = lambda a: a.ctypes.data_as(lktree.C.c_void_p)

        def new_call():
            t.L.Get_All_Ancestral_Probs(t.tree, lktree._dp(out))
            lktree._raise_if_error()

        def kernel_ms():
            new_call()
            ms, calls = t.inst.profile_read_node_posteriors()
            assert calls == 1
            return ms

        def old_route():
            for idx in bufs:
                assert L.phyhip_get_partials(iid, idx, -1, dp(part)) >= 0
                assert L.phyhip_get_scale_factors(iid, idx, dp(scal)) >= 0

        s_new, _ = medians(new_call, warm, reps)
        sums = out.sum(axis=2)
        t.inst.profile(1)
        t.inst.profile_read_node_posteriors()
        _, ms_kernel = medians(kernel_ms, warm, reps)
        t.inst.profile(0)
        s_old, _ = medians(old_route, warm, reps)
        # algorithmic bytes of (b): of the 3(n - 2) sides the nodes read, n are tips (one byte per pattern), 2n - 6 are buffers (C x S
        # doubles + a scale int); the n buffers that face a tip are read by no node
        internal_sides = 3 * (n - 2) - n
        alg = P * (internal_sides * (Cc * S * 8 + 4) + n * 1 + (n - 2) * S * 8)
        return dict(workload=name, taxa=n, patterns=P, states=S, categories=Cc, nodes=n - 2,
                    ms_new_call=s_new * 1e3, ms_kernel=ms_kernel, ms_old_route_downloads=s_old * 1e3,
                    result_MB=(n - 2) * P * S * 8 / 1e6, old_route_MB=len(bufs) * P * (Cc * S * 8 + 4) / 1e6, old_route_buffers=len(bufs),
                    kernel_algorithmic_MB=alg / 1e6, kernel_TB_per_s=alg / (ms_kernel * 1e-3) / 1e12,
                    kernel_share_of_8TBps=alg / (ms_kernel * 1e-3) / HBM_BYTES_PER_S,
                    worst_sum_deviation=float(np.max(np.abs(sums - 1.0))))
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ancestral_posteriors.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    rows = [one("cfg2_nt_100x50k", a.warm, a.reps), one("cfg3_aa_200x10k", a.warm, a.reps)]
    with open(a.out, "w") as f:
        f.write("# Marginal ancestral state posteriors: device route against the download route\n\n"
                "`tools/ancestral_timing.py` on one MI355X, one process, after `Set_Both_Sides(YES); Lk(NULL)`; medians of %d after %d warm-ups.\n\n"
                "- (a) `Get_All_Ancestral_Probs`: one `phyhip_calculate_node_state_posteriors` call for all n - 2 nodes, download of the result included (host wall time).\n"
                "- (b) its kernel alone, HIP events; bytes / time counts three side reads, three scale reads and one result write per (node, pattern), against 8 TB/s.\n"
                "- (c) the route it replaces, downloads only (`phyhip_get_partials` + `phyhip_get_scale_factors` for every internal side buffer, no host arithmetic): a lower bound of that route.\n\n"
                "| workload | nodes | (a) new call ms | (b) kernel ms | (c) old route, downloads only ms | (c) / (a) | result MB | old route MB (buffers) | kernel bytes MB | kernel TB/s | of 8 TB/s |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n" % (a.reps, a.warm))
        for r in rows:
            f.write("| %s (%d x %d patterns x %d states, %d categories) | %d | %.2f | %.3f | %.2f | %.1f | %.0f | %.0f (%d) | %.0f | %.2f | %.0f %% |\n" % (
                r["workload"], r["taxa"], r["patterns"], r["states"], r["categories"], r["nodes"], r["ms_new_call"], r["ms_kernel"],
                r["ms_old_route_downloads"], r["ms_old_route_downloads"] / r["ms_new_call"], r["result_MB"], r["old_route_MB"],
                r["old_route_buffers"], r["kernel_algorithmic_MB"], r["kernel_TB_per_s"], 100.0 * r["kernel_share_of_8TBps"]))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
