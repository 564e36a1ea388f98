"""The parsimony regraft scan against the route it replaces, one device, one process, through the C ABI with prebuilt ctypes arrays.
    scan    ONE phyhip_calculate_regraft_parsimony over K candidates of one pruned subtree
    route   per candidate: phyhip_update_partial_parsimony with one operation (into a spare plane) and
            phyhip_calculate_edge_parsimony, which launches, waits and reads 8 bytes back
Random trees at 54 x 382 nt, 37 x 429 aa, 24 x 2 048 nt and 500 x 100 000 nt (columns drawn independently: every column a pattern,
all weights 1), K in {1, 8, 64, 512}, both modes.  The candidates are target edges of the tree drawn with a fixed seed (with
repeats where K exceeds the edges) and one subtree vector, as one scan of Spr_Pars has.  The two routes alternate call by call;
every call ends with the host holding the sums; host wall time, median and the 10th / 90th percentile of --reps calls after --warm
warm calls.  The scan's kernel time is read from phyhip_profile_read_regraft_parsimony in a pass of its own.  The sums of both
routes are compared before anything is timed.  Prints one JSON line per (shape, mode, K).
    python tools/pars_regraft_bench.py [--reps 200] [--warm 20] [--shapes example_nt,example_aa,nt_24x2048,cfg5] [--ks 1,8,64,512]
                                       [--no-route] [--label TEXT]
PHYHIP_LIBDIR names another build of the library (one compiled with -DPHYHIP_PARS_SLAB_FACTOR=2 or 8: the slab-count alternatives of
profiles/parsimony_regraft_scan.md); --label goes into every line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from phyml_amd import capi

SHAPES = {"example_nt": (54, 382, 4), "example_aa": (37, 429, 20), "nt_24x2048": (24, 2048, 4), "cfg5": (500, 100000, 4)}


class Operation(C.Structure):
    """phyhip_parsimony_operation"""
    _fields_ = [("destination", C.c_int), ("child1", C.c_int), ("child2", C.c_int)]


def random_tree(n, rng):
    """neighbour lists of a random unrooted binary topology: tips 0..n-1, inner nodes n..2n-3"""
    nxt, edges = n + 1, [(n, 0), (n, 1), (n, 2)]
    for t in range(3, n):
        a, b = edges.pop(rng.randint(len(edges)))
        edges += [(nxt, a), (nxt, b), (nxt, t)]
        nxt += 1
    nb = [[] for _ in range(2 * n - 2)]
    for a, b in edges:
        nb[a].append(b); nb[b].append(a)
    return edges, nb


def all_vectors(n, edges, nb):
    """operations (dest, child1, child2) that fill the vector of every edge side that ends in an inner node, in dependency order
    (an explicit stack: 500 taxa make a deep tree), and {(a, d): buffer} -- the vector behind d seen from a"""
    ops, memo, nxt = [], {}, n
    for a, b in edges:
        for root in ((a, b), (b, a)):
            stack = [root]
            while stack:
                x, d = stack[-1]
                if d < n or (x, d) in memo:
                    stack.pop()
                    continue
                kids = [c for c in nb[d] if c != x]
                todo = [(d, c) for c in kids if c >= n and (d, c) not in memo]
                if todo:
                    stack.extend(todo)
                    continue
                memo[(x, d)] = nxt
                ops.append((nxt, kids[0] if kids[0] < n else memo[(d, kids[0])], kids[1] if kids[1] < n else memo[(d, kids[1])]))
                nxt += 1
                stack.pop()
    return ops, memo, nxt


def quantiles(ts):
    ts = np.asarray(ts) * 1e6
    return [round(float(np.percentile(ts, q)), 2) for q in (50, 10, 90)]


def run_shape(name, general, ks, reps, warm, with_route, label):
    n, P, ns = SHAPES[name]
    rng = np.random.RandomState(n + P)
    edges, nb = random_tree(n, rng)
    ops, memo, nbuf = all_vectors(n, edges, nb)
    spare = nbuf
    inst = capi.Instance(n, nbuf + 1, ns, P, 2 * n, 1, device=0)
    L = inst.L
    try:
        inst.set_pattern_weights(np.ones(P))
        states = rng.randint(ns, size=(n, P))
        for t in range(n):
            inst.set_tip_partials(t, np.eye(ns)[states[t]])
        step = rng.randint(1, 4, size=(ns, ns)); np.fill_diagonal(step, 0)
        inst.set_parsimony(general, step if general else None)
        inst.update_partial_parsimony(ops)
        vec = lambda a, d: d if d < n else memo[(a, d)]
        sa, sd = edges[rng.randint(len(edges))]
        sub = vec(sa, sd)
        for K in ks:
            targets = [edges[i] for i in rng.randint(len(edges), size=K)]
            cands = [(vec(y, x), vec(x, y), sub) for x, y in targets]
            arr = (capi.ParsimonyCandidate * K)(*[capi.ParsimonyCandidate(*c) for c in cands])
            out = (C.c_longlong * K)()
            route_ops = [Operation(spare, c[0], c[1]) for c in cands]
            route_out = (C.c_longlong * K)()
            one = C.c_longlong(0)

            def scan():
                rc = L.phyhip_calculate_regraft_parsimony(inst.id, arr, K, -1, out)
                assert rc == 0, rc

            def route():
                for k in range(K):
                    L.phyhip_update_partial_parsimony(inst.id, C.byref(route_ops[k]), 1)
                    rc = L.phyhip_calculate_edge_parsimony(inst.id, spare, sub, C.byref(one))
                    assert rc == 0, rc
                    route_out[k] = one.value

            scan()
            route()
            assert list(out) == list(route_out), (name, general, K)
            for _ in range(warm):
                scan()
                if with_route:
                    route()
            t_scan, t_route = [], []
            for _ in range(reps):
                t0 = time.perf_counter(); scan(); t_scan.append(time.perf_counter() - t0)
                if with_route:
                    t0 = time.perf_counter(); route(); t_route.append(time.perf_counter() - t0)
            inst.profile(1)
            inst.profile_read_regraft_parsimony()
            for _ in range(reps):
                scan()
            ms, calls, nc = inst.profile_read_regraft_parsimony()
            inst.profile(0)
            assert calls == reps and nc == reps * K
            slabs, size = capi.pars_regraft_slabs(K, P, inst.details.computeUnits)   # (of the default factor)
            rec = {"shape": name, "taxa": n, "patterns": P, "states": ns, "mode": "step_matrix" if general else "fitch", "K": K,
                   "scan_call_us_p50_p10_p90": quantiles(t_scan), "scan_kernel_us": round(ms * 1e3 / reps, 2),
                   "scan_us_per_candidate": round(quantiles(t_scan)[0] / K, 3), "default_slabs": [slabs, size], "reps": reps,
                   "compute_units": inst.details.computeUnits, "lib": os.path.relpath(capi.LIB_DIR, ROOT), "label": label}
            if with_route:
                rec["route_call_us_p50_p10_p90"] = quantiles(t_route)
                rec["route_us_per_candidate"] = round(quantiles(t_route)[0] / K, 3)
                rec["route_over_scan"] = round(quantiles(t_route)[0] / quantiles(t_scan)[0], 2)
            print(json.dumps(rec), flush=True)
    finally:
        inst.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--shapes", default="example_nt,example_aa,nt_24x2048,cfg5")
    ap.add_argument("--ks", default="1,8,64,512")
    ap.add_argument("--no-route", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        for general in (False, True):
            run_shape(name, general, [int(k) for k in a.ks.split(",")], a.reps, a.warm, not a.no_route, a.label)


if __name__ == "__main__":
    main()
