"""The mixture regraft scan (phyhip_calculate_mixture_regraft_log_likelihoods) against the per-candidate route on the SAME library: K
candidates of one subtree -- random target edges of the evaluated class trees, random lengths -- timed two ways, K = 1, 8, 64, 512:
    scan      one call of the scan (the ctypes record array and the per-class tables built outside the timed region);
    existing  the same candidates one by one through the existing entry points: per candidate, in every class instance,
              phyhip_update_transition_matrices of the three lengths and phyhip_update_partials into the spare buffer, then one
              phyhip_calculate_mixture_log_likelihood over the class list -- issued from Python, every ctypes array prebuilt: the
              interpreter's share (2 x classes + 1 foreign calls per candidate) is inside this column.
Shapes: the two mixture fixtures' own -- tests/golden/mixture_nt4.phyg (54 taxa x 382 patterns, four nucleotide classes) and
mixture_lg4x.phyg (37 x 429, the four LG4X classes).  Every shape runs in a child process of its own under its own time limit; a
child that runs out of time or fails is reported as such and nothing more is started.  Reported per K: min and median of --reps plain
runs after one warm run, and -- from phyhip_profile_read_mixture_regraft, in a profiled run of its own -- the kernel time of the scan.
    python tools/mixture_regraft_timing.py [--reps 9] [--shapes nt4,lg4x] [--limit 120] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KS = (1, 8, 64, 512)
SHAPES = ("nt4", "lg4x")


def make_trees(shape):
    import numpy as np
    from phyml_amd import lktree, phyg, replay
    d = phyg.load(os.path.join(ROOT, "tests", "golden", "mixture_%s.phyg" % shape))
    models, factors = replay.mixture_classes(d)
    n, P, S = int(d["n_otu"][0]), int(d["n_pattern"][0]), int(d["ns"][0])
    tv, _, _ = replay.tips_from_masks(d["tip_mask"], S)
    trees = []
    for md in models:
        t = lktree.LkTree(n, d["edge_left"], d["edge_rght"], d["edge_len"], P, S, 1, host_pmat=False)
        t.tip_root = 0
        t.set_model(md["pi"], md["gamma_rr"], md["gamma_r_proba"], md["e_val"], md["r_e_vect"], md["l_e_vect"], float(md["l_min"][0]),
                    float(md["l_max"][0]), float(md["br_len_mult"][0]), 1, 0, 0.0)
        t.Make_Tree_For_Lk(d["wght"], None)
        t.set_tips(tip_partials=tv)
        t.Set_Both_Sides(True)
        t.Lk(None)
        trees.append(t)
    sums = (float(d["r_mat_weight_sum"][0]), float(d["e_frq_weight_sum"][0]), float(d["sum_probas"][0]))
    return trees, factors, sums, np.asarray(d["edge_len"], dtype=np.float64)


def candidates(t, lens, K, seed=5):
    """K records of one subtree: (child 1, child 2, subtree, flags, three lengths); the targets are edges with two internal ends"""
    import numpy as np
    rng = np.random.default_rng(seed)
    inner = [e for e in range(t.ne) if not t.edge(e).contents.left.contents.tax and not t.edge(e).contents.rght.contents.tax]
    sub_edge = inner[0]
    sub = t.side_buffer(sub_edge, 1)
    out = []
    for k in range(K):
        e = inner[1 + int(rng.integers(len(inner) - 1))]
        f = float(rng.uniform(0.1, 0.9))
        out.append((t.side_buffer(e, 0), t.side_buffer(e, 1), sub, 0, f * lens[e] + 1e-4, (1.0 - f) * lens[e] + 1e-4,
                    float(lens[sub_edge]) * float(rng.uniform(0.5, 1.5))))
    return out


def child(shape, reps):
    import numpy as np
    from phyml_amd import capi
    trees, factors, sums, lens = make_trees(shape)
    try:
        L, n = capi.load(), len(trees)
        t0 = trees[0]
        ids = (C.c_int * n)(*[t.tree.contents.b_inst for t in trees])
        eig = (C.c_int * n)(*([0] * n))
        da = lambda v: (C.c_double * n)(*[float(x) for x in v])
        proba, rw, ew = da([f[0] for f in factors]), da([f[1] for f in factors]), da([f[2] for f in factors])
        rs, es, sp = (C.c_double(x) for x in sums)
        spare, sm = t0.spare_p_lk_idx, t0.spare_Pij_idx
        assert all(t.spare_p_lk_idx == spare and t.spare_Pij_idx == sm for t in trees)
        midx = (C.c_int * 3)(sm, sm + 1, sm + 2)
        par, pms = (C.c_int * n)(*([spare] * n)), (C.c_int * n)(*([sm + 2] * n))
        row = dict(shape=shape, taxa=t0.n, patterns=t0.P, states=t0.S, classes=n)
        for K in KS:
            cands = candidates(t0, lens, K)
            arr = (capi.RegraftCandidate * K)(*[capi.RegraftCandidate(*c) for c in cands])
            out = np.zeros(K)
            # the per-candidate route's arrays, prebuilt
            lens3 = [(C.c_double * 3)(c[4], c[5], c[6]) for c in cands]
            ops = [(capi.Operation * 1)(capi.Operation(spare, -1, -1, c[0], sm, c[1], sm + 1)) for c in cands]
            chi = [(C.c_int * n)(*([c[2]] * n)) for c in cands]
            one = C.c_double(0.0)
            ref = np.zeros(K)

            def scan():
                a = time.perf_counter()
                capi._chk(L.phyhip_calculate_mixture_regraft_log_likelihoods(ids, n, eig, arr, K, -1, proba, rw, ew, rs, es, sp, capi._ptr(out), None))
                return time.perf_counter() - a

            def loop():
                a = time.perf_counter()
                for k in range(K):
                    for i in ids:
                        L.phyhip_update_transition_matrices(i, 0, midx, None, None, lens3[k], 3)
                        L.phyhip_update_partials(i, ops[k], 1, -1)
                    capi._chk(L.phyhip_calculate_mixture_log_likelihood(ids, n, par, chi[k], pms, proba, rw, ew, rs, es, sp, C.byref(one)))
                    ref[k] = one.value
                return time.perf_counter() - a
            scan(); loop()
            assert np.max(np.abs(out - ref) / np.abs(ref)) < 1e-10, (shape, K, out[:3], ref[:3])
            ts = [scan() for _ in range(reps)]
            tl = [loop() for _ in range(max(3, reps // 3) if K == 512 else reps)]
            row["scan_min_us_K%d" % K], row["scan_med_us_K%d" % K] = min(ts) * 1e6, float(np.median(ts)) * 1e6
            row["loop_min_us_K%d" % K], row["loop_med_us_K%d" % K] = min(tl) * 1e6, float(np.median(tl)) * 1e6
            t0.inst.profile(1); t0.inst.profile_read_mixture_regraft()
            scan()
            ms, calls, nc = t0.inst.profile_read_mixture_regraft()
            t0.inst.profile(0)
            assert calls == 1 and nc == K
            row["scan_kernel_us_K%d" % K] = ms * 1e3
            print(json.dumps({k: v for k, v in row.items() if k.endswith("K%d" % K)}), file=sys.stderr, flush=True)
        print(json.dumps(row), flush=True)
    finally:
        for t in trees:
            t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=int, default=120, help="seconds per child process")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    rows, rc = [], 0
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            rows.append(dict(shape=shape, timed_out=a.limit))
            print(json.dumps(rows[-1]), flush=True)
            print("a run went over its time limit: nothing more is started", file=sys.stderr)
            rc = 1
            break
        if r.returncode != 0:
            rows.append(dict(shape=shape, failed=r.returncode))
            print(json.dumps(rows[-1]), flush=True)
            print("a run failed: nothing more is started", file=sys.stderr)
            rc = 1
            break
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
