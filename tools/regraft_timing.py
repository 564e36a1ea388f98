"""The regraft scan (phyhip_calculate_regraft_log_likelihoods) against the per-candidate route on the SAME library: K candidates of one
subtree -- random target edges of an evaluated tree, random lengths -- timed three ways, K = 1, 8, 64, 512:
    scan      one call of the scan (the ctypes record array built outside the timed region);
    existing  the same candidates one by one through the existing entry points -- per candidate two matrix rebuilds, one
              phyhip_update_partials into the spare buffer, a third rebuild and phyhip_calculate_edge_log_likelihoods -- in ONE C loop
              (Replay_Surface_Trace of the host layer), served by the resident evaluators where they serve this pattern;
    launched  that same loop with PHYHIP_RESIDENT=0: every candidate a kernel launch and a wait.
Shapes: the two committed examples (nucleic_gtr_g4: 54 taxa x 382 patterns; proteic_lg_g4: 37 x 429, 20 states), a synthetic 24-taxon
tree of 2 048 nucleotide patterns, and 500 taxa x 100 000 nucleotide patterns.  Every (shape, resident on / off) pair runs in a child
process of its own under its own time limit (the switch is read when the instance is made); a child that runs out of time is
reported as such and the next one starts.  Reported: medians of --reps plain runs after one warm run, and -- from
phyhip_profile_read_regraft, in a profiled run of its own -- the kernel time of the scan.
    python tools/regraft_timing.py [--reps 7] [--shapes nt54,aa37,nt2048,nt100k] [--limit 240] [--json out.json]"""
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
SHAPES = ("nt54", "aa37", "nt2048", "nt100k")


def make_tree(shape):
    import numpy as np
    from phyml_amd import lktree, phyg, synth, workloads
    if shape in ("nt54", "aa37"):
        from gpu_common import device_tree_from_golden
        d = phyg.load(os.path.join(ROOT, "tests", "golden", ("nucleic_gtr_g4" if shape == "nt54" else "proteic_lg_g4") + ".phyg"))
        t, _ = device_tree_from_golden(d)
        return t, np.asarray(d["edge_len"], dtype=np.float64)
    n, P = (24, 2048) if shape == "nt2048" else (500, 100000)
    tree = synth.random_tree(n, 7, 0.02, 0.3)
    st = synth.simulate_states(tree, P, 4, 7)
    blk = workloads.model_block("model_gtr_g4")
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, 4, int(blk["ncatg"][0]), device=0)
    t.set_model(blk["pi"], blk["gamma_rr"], blk["gamma_r_proba"], blk["e_val"], blk["r_e_vect"], blk["l_e_vect"],
                float(blk["l_min"][0]), float(blk["l_max"][0]), 1.0, 1)
    t.Make_Tree_For_Lk(np.ones(P))
    t.set_tips(tip_states=st.astype(np.int32))
    return t, np.asarray(tree.edge_len, dtype=np.float64)


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


def as_trace(t, cands):
    import numpy as np
    from phyml_amd import replay
    sb, sm = t.spare_p_lk_idx, t.spare_Pij_idx
    rec = {k: [] for k in ("kind", "a", "b", "c", "d", "e", "x")}

    def push(kind, a=0, b=0, c=0, d=0, e=0, x=0.0):
        for k, v in zip(("kind", "a", "b", "c", "d", "e", "x"), (kind, a, b, c, d, e, x)):
            rec[k].append(v)
    for (c1, c2, sub, flags, l1, l2, l3) in cands:
        push(replay.SET_PMAT, a=sm, x=l1)
        push(replay.SET_PMAT, a=sm + 1, x=l2)
        push(replay.UPDATE, a=sb, b=c1, c=sm, d=c2, e=sm + 1)
        push(replay.SET_PMAT, a=sm + 2, x=l3)
        push(replay.EDGE_LNL, a=sb, b=sub, c=sm + 2)
    return {k: np.array(v, dtype=np.float64 if k == "x" else np.int32) for k, v in rec.items()}


def child(shape, reps):
    import numpy as np
    from phyml_amd import capi
    t, lens = make_tree(shape)
    try:
        t.tree.contents.host_pmat = 0   # the per-candidate route builds its matrices on the device too
        t.Set_Both_Sides(True)
        t.Lk(None)
        row = dict(shape=shape, taxa=t.n, patterns=t.P, states=t.S, resident=os.environ.get("PHYHIP_RESIDENT", "1") != "0")
        fn = t.inst.L.phyhip_calculate_regraft_log_likelihoods
        for K in KS:
            cands = candidates(t, lens, K)
            arr = (capi.RegraftCandidate * K)(*[capi.RegraftCandidate(*c) for c in cands])
            out = np.zeros(K)
            tr = as_trace(t, cands)

            def scan():
                a = time.perf_counter()
                capi._chk(fn(t.inst.id, 0, arr, K, -1, capi._ptr(out), None))
                return time.perf_counter() - a

            def loop():
                a = time.perf_counter()
                got, _ = t.Replay_Surface_Trace(tr)
                return time.perf_counter() - a, got[4::5]
            scan(); ref = loop()[1]
            assert np.max(np.abs(out - ref) / np.abs(ref)) < 1e-10, (shape, K)
            row["scan_us_K%d" % K] = float(np.median([scan() for _ in range(reps)])) * 1e6
            row["loop_us_K%d" % K] = float(np.median([loop()[0] for _ in range(reps)])) * 1e6
            t.inst.profile(1); t.inst.profile_read_regraft()
            scan()
            ms, calls, n = t.inst.profile_read_regraft()
            t.inst.profile(0)
            row["scan_kernel_us_K%d" % K] = ms * 1e3
            print(json.dumps({k: v for k, v in row.items() if k.endswith("K%d" % K)}), file=sys.stderr, flush=True)
        print(json.dumps(row), flush=True)
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    rows = []
    for shape in a.shapes.split(","):
        for resident in ("1", "0"):
            env = dict(os.environ, PHYHIP_RESIDENT=resident)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                rows.append(dict(shape=shape, resident=resident == "1", timed_out=a.limit))
                print(json.dumps(rows[-1]), flush=True)
                print("a run went over its time limit: nothing more is started", file=sys.stderr)
                break
            if r.returncode != 0:
                rows.append(dict(shape=shape, resident=resident == "1", failed=r.returncode))
                print(json.dumps(rows[-1]), flush=True)
                print("a run failed: nothing more is started", file=sys.stderr)
                if a.json:
                    json.dump(rows, open(a.json, "w"), indent=1)
                return 1
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
        else:
            continue
        break
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
