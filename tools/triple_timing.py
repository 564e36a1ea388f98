"""Triple_Dist at K nodes in one device call (phyhip_optimise_triples) against the chain on the SAME library: the host layer's
Triple_Dist -- Update_PMat_At_Given_Edge, Update_Partial_Lk and Br_Len_Opt driving dLk() from the host, one C function per node, served
by the resident evaluators where they serve this pattern -- which runs on the entry points that were there before this call, i.e. it is
what the parent commit can do.  K = 1, 8, 64 internal nodes of an evaluated tree (taken in turn, round again where the tree has
fewer), each from the tree's own lengths scaled by --scales (1: searches of a few probes, as behind an accepted move; 0.05: long
walks), timed two ways:
    call    one phyhip_optimise_triples over the K candidates (the ctypes record array built outside the timed region);
    chain   Triple_Dist(a, tree) at the same K nodes one after the other; the three lengths are put back between nodes outside the
            timed region (the matrix refresh that goes with it is queued work the next Triple_Dist overwrites).  One foreign call of the C function
            per node, each inside its own pair of clock readings: the interpreter's few microseconds per node are in this column.
Shapes: the two committed examples (nucleic_gtr_g4: 54 taxa x 382 patterns; proteic_lg_g4: 37 x 429, 20 states) and a synthetic
24-taxon tree of 2 048 nucleotide patterns.  Each shape runs in a child process of its own under its own time limit; a child that
runs out of time or fails is reported and nothing more is started.  Reported: medians of --reps runs after one warm run, the evaluations
the call took, and -- from phyhip_profile_read_triples, in a profiled run of its own -- the kernel time of the call.
    python tools/triple_timing.py [--reps 7] [--shapes nt54,aa37,nt2048] [--scales 1,0.05] [--limit 240] [--json out.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KS = (1, 8, 64)
SHAPES = ("nt54", "aa37", "nt2048")


def candidate(t, a, factor):
    from phyml_amd import capi
    nd = t.node(a).contents
    x, fl, ln = [], 0, []
    for i in range(3):
        b = nd.b[i].contents
        if b.left.contents.num == a:
            fl |= capi.triple_node_is_left(i)
            x.append(b.p_lk_tip_idx if b.rght.contents.tax else b.p_lk_rght_idx)
        else:
            x.append(b.p_lk_left_idx)
        ln.append(min(b.l * factor, 90.0))
    return x, fl, ln


def child(shape, reps, scales):
    import ctypes as C
    import numpy as np
    from phyml_amd import capi
    from regraft_timing import make_tree
    t, lens = make_tree(shape)
    try:
        t.tree.contents.host_pmat = 0   # the chain builds its matrices on the device too
        t.Set_Both_Sides(True)
        t.Lk(None)
        row = dict(shape=shape, taxa=t.n, patterns=t.P, states=t.S)
        fn = t.inst.L.phyhip_optimise_triples
        inner = list(range(t.n, 2 * t.n - 2))
        for factor in scales:
            for K in KS:
                nodes = [inner[k % len(inner)] for k in range(K)]
                cands = [candidate(t, a, factor) for a in nodes]
                arr = (capi.TripleCandidate * K)(*[capi.TripleCandidate((C.c_int * 3)(*x), fl, (C.c_double * 3)(*ln)) for x, fl, ln in cands])
                out = (capi.TripleResult * K)()
                edges = [[t.node(a).contents.b[i].contents.num for i in range(3)] for a in nodes]

                def call():
                    a = time.perf_counter()
                    capi._chk(fn(t.inst.id, arr, K, capi.BRENT_IT_MAX, C.c_double(1e-3), -1, out))
                    return time.perf_counter() - a

                def chain():
                    total, got = 0.0, []
                    for a, e, (x, fl, ln) in zip(nodes, edges, cands):
                        for b, l in zip(e, ln):
                            t.edge(b).contents.l = l
                        nd = t.node(a)
                        s = time.perf_counter()
                        t.L.Triple_Dist(nd, t.tree)
                        total += time.perf_counter() - s
                        got.append(t.tree.contents.n_tot_bl_opt)
                        for b in e:
                            t.edge(b).contents.l = float(lens[b])
                            t.Update_PMat_At_Given_Edge(b)
                        for b in e:
                            t.Update_Partial_Lk(b, a)
                    return total, got
                call()
                n0 = t.n_tot_bl_opt
                steps = chain()[1][-1] - n0
                evals = sum(sum(out[k].evaluations) for k in range(K))
                # the two routes took the same searches (steps: the evaluations after each search's first, plus the walks that left the bracket)
                assert steps == sum(ev - 1 + (1 if st in (1, 2) else 0) for k in range(K) for ev, st in zip(out[k].evaluations, out[k].status)), (shape, K)
                tag = "s%g_K%d" % (factor, K)
                row["call_us_" + tag] = float(np.median([call() for _ in range(reps)])) * 1e6
                row["chain_us_" + tag] = float(np.median([chain()[0] for _ in range(reps)])) * 1e6
                row["evaluations_" + tag] = evals
                t.inst.profile(1); t.inst.profile_read_triples()
                call()
                ms, calls, n = t.inst.profile_read_triples()
                t.inst.profile(0)
                row["call_kernel_us_" + tag] = ms * 1e3
                print(json.dumps({k: v for k, v in row.items() if k.endswith(tag)}), file=sys.stderr, flush=True)
        print(json.dumps(row), flush=True)
    finally:
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--scales", default="1,0.05")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    scales = [float(x) for x in a.scales.split(",")]
    if a.child:
        return child(a.child, a.reps, scales)
    rows, rc = [], 0
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--scales", a.scales]
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
