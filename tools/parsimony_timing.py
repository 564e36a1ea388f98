"""Parsimony on the device: what a call costs, at the benchmark shapes and at the 54 x 382 example, both modes, one device, one process.
    (a) Pars(NULL) with both sides     3(n - 2) operations and the score of a_nodes[0]->b[0]: ONE phyhip_update_partial_parsimony per
                                       traversal and ONE phyhip_calculate_edge_parsimony -- host wall time of the C host layer's call,
                                       the download of site_pars included
    (b) Update_Pars_At_Given_Edge(b)   two operations and the score of an internal edge (an SPR candidate's call pattern)
and the kernel time of each (HIP events, phyhip_profile_read_parsimony).  The bytes a launch moves are computed here from the operation
list: per operation and pattern 8 B (Fitch) or 4 S B (step matrix) for each inner child that is not the previous operation's result,
1 B for each tip child, and as much written as an inner child holds; the score reads its two sides, the weight, and writes 4 B.
Bytes over kernel time are reported against 6.3 TB/s (what a streaming kernel reaches on this part).  Median of --reps after --warm
warm calls, every call ending in the host having the score.
    python tools/parsimony_timing.py [--reps 20] [--warm 5] [--shapes cfg2,cfg3,cfg5,example]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from phyml_amd import lktree, synth, workloads

ACHIEVABLE_BYTES_PER_S = 6.3e12
SHAPES = {"cfg2": (100, 50000, 4), "cfg3": (200, 10000, 20), "cfg5": (500, 100000, 4), "example": (54, 382, 4)}


def medians(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts, vs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        v = fn()
        ts.append(time.perf_counter() - t0)
        vs.append(v)
    return float(np.median(ts)), float(np.median(vs))


def both_sides_ops(t):
    """the operations Pars(NULL) queues with both_sides == YES, as (dest, child1, child2) -- the host layer's own resolution restated
    over the ctypes mirror (src/pars.c:56-93)"""
    n = t.n
    num = lambda p: p.contents.num

    def child(d, b):
        e = b.contents
        if d == num(e.left):
            return e.p_lk_tip_idx if e.rght.contents.tax else e.p_lk_rght_idx
        return e.p_lk_left_idx

    def op(b, d):
        nd, e = t.node(d).contents, b.contents
        kids = [child(d, nd.b[i]) for i in range(3) if nd.b[i].contents.num != e.num]
        return (e.p_lk_left_idx if d == num(e.left) else e.p_lk_rght_idx, kids[0], kids[1])

    ops, stack = [], [(0, num(t.node(0).contents.v[0]), 0, -1)]
    while stack:                                    # post-order
        a, d, i, dr = stack.pop()
        if d < n:
            continue
        nd = t.node(d).contents
        if i < 3:
            v = num(nd.v[i])
            stack.append((a, d, i + 1, i if v == a else dr))
            if v != a:
                stack.append((d, v, 0, -1))
            continue
        ops.append(op(nd.b[dr], d))
    stack = [(0, num(t.node(0).contents.v[0]), 0)]
    while stack:                                    # pre-order
        a, d, i = stack.pop()
        if d < n or i == 3:
            continue
        nd = t.node(d).contents
        stack.append((a, d, i + 1))
        v = num(nd.v[i])
        if v != a:
            ops.append(op(nd.b[i], d))
            stack.append((d, v, 0))
    return ops


def launch_bytes(ops, score, n, P, S, general):
    """bytes one launch moves for `ops` then the score of edge `score` (None: none), by the rule of the module docstring"""
    inner = 4 * S if general else 8
    total, prev = 0, -1
    for d, c1, c2 in ops:
        for c in (c1, c2):
            total += 1 if c < n else (0 if (c == prev and not general) else inner)
        total += inner
        prev = d
    if score is not None:
        total += sum(1 if c < n else inner for c in score) + 8 + 4
    return total * P


def one(name, warm, reps):
    n, P, S = SHAPES[name]
    tree = synth.random_tree(n, 7, 0.02, 0.3)
    st = synth.simulate_states(tree, P, S, 7)
    blk = workloads.model_block("model_gtr_g4" if S == 4 else "model_lg_g4")
    Cc = int(blk["ncatg"][0])
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, S, Cc, device=0)
    rows = []
    try:
        t.set_model(blk["pi"], blk["gamma_rr"], blk["gamma_r_proba"], blk["e_val"], blk["r_e_vect"], blk["l_e_vect"],
                    float(blk["l_min"][0]), float(blk["l_max"][0]), 1.0, 1)
        t.Make_Tree_For_Lk(np.ones(P))
        t.set_tips(tip_states=st.astype(np.int32))
        t.Set_Both_Sides(True)
        ops = both_sides_ops(t)
        inner_edge = next(e for e in range(t.ne) if not t.edge(e).contents.rght.contents.tax)
        eb = t.edge(inner_edge).contents
        root_b = t.node(0).contents.b[0].contents
        edge_ops = [o for o in ops if o[0] == eb.p_lk_left_idx][:1] + [o for o in ops if o[0] == eb.p_lk_rght_idx][:1]
        for general in (False, True):
            # (20 states: the 0/1 matrix -- the reference's amino-acid table is the caller's to pass in; the kernel's work is the same)
            t.Make_Tree_For_Pars(general)
            full = t.Pars(None)

            def pars_null():
                return t.Pars(None)

            def edge_call():
                return t.Update_Pars_At_Given_Edge(inner_edge)

            def kernel_of(fn):
                def f():
                    fn()
                    ms, launches, _ = t.inst.profile_read_parsimony()
                    assert launches == 1, launches
                    return ms
                return f

            s_null, v = medians(pars_null, warm, reps)
            assert v == full
            s_edge, v = medians(edge_call, warm, reps)
            assert general or v == full                      # (Fitch: the length is the same at every edge)
            t.inst.profile(1)
            t.inst.profile_read_parsimony()
            _, ms_null = medians(kernel_of(pars_null), warm, reps)
            _, ms_edge = medians(kernel_of(edge_call), warm, reps)
            t.inst.profile(0)
            b_null = launch_bytes(ops, (root_b.p_lk_left_idx, root_b.p_lk_tip_idx), n, P, S, general)
            b_edge = launch_bytes(edge_ops, (eb.p_lk_left_idx, eb.p_lk_rght_idx), n, P, S, general)
            plane = (4 * S if general else 8) * P
            rows.append(dict(shape=name, taxa=n, patterns=P, states=S, mode="step matrix" if general else "Fitch", c_pars=int(full),
                             operations=len(ops), pars_null_wall_us=s_null * 1e6, pars_null_kernel_us=ms_null * 1e3,
                             pars_null_MB=b_null / 1e6, pars_null_TB_per_s=b_null / (ms_null * 1e-3) / 1e12,
                             pars_null_share_of_achievable=b_null / (ms_null * 1e-3) / ACHIEVABLE_BYTES_PER_S,
                             pars_null_ns_per_pattern_update=ms_null * 1e6 / ((len(ops) + 1.0) * P),
                             edge_wall_us=s_edge * 1e6, edge_kernel_us=ms_edge * 1e3, edge_MB=b_edge / 1e6,
                             edge_TB_per_s=b_edge / (ms_edge * 1e-3) / 1e12, working_set_MB=plane * 3 * (n - 2) / 1e6 + n * P / 1e6))
            print(json.dumps(rows[-1]))
            sys.stdout.flush()
    finally:
        t.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--shapes", default="example,cfg2,cfg3,cfg5")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        one(name, a.warm, a.reps)


if __name__ == "__main__":
    main()
