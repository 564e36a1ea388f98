"""Br_Len_Opt on the device against the host-driven chain on the SAME library: one pass of the host layer's Br_Len_Opt over every edge
of a tree from the tree's own lengths (each edge restored afterwards), once with the search in one device call
(phyhip_optimise_edge_length) and once with force_host_chain (the same search, one phyhip_calculate_eigen_lnl_dlnl round trip per
probe), in the same process, --reps passes each after one warm pass.  Per route: the median pass time, the time per call by the
call's evaluation count (1-2, 3-8, > 8), and -- device route, from phyhip_profile_read_edge_length in a profiled pass of its own --
the kernel time per evaluation.  A pass times Br_Len_Opt whole: Lk(b) with update_eigen_lr, the search, the matrix refresh; the two
routes differ in the search alone.
    trees: the two committed examples (nucleic_gtr_g4: 54 taxa x 382 patterns, proteic_lg_g4: 37 x 429) and a synthetic 4-state one
    --sweep: 4 states, 4 categories, 24 taxa, P = 512 ... 131 072: where the one-workgroup call stops beating the chain.  The call
    refuses more than capi.BRLEN_MAX_PATTERNS patterns, so the sweep runs on the diag build (phyml_amd/lib_diag, the same kernels)
    with its switch PHYHIP_BRLEN_MAX_PATTERNS raised.
The device route is asked for (force_device) whatever the host layer's own rule would choose; "rule" is a third pass with that rule.
    python tools/brlen_timing.py [--reps 5] [--sweep] [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if "--sweep" in sys.argv:   # (before the bindings read it)
    os.environ.setdefault("PHYHIP_LIBDIR", os.path.join(ROOT, "phyml_amd", "lib_diag"))
    os.environ.setdefault("PHYHIP_BRLEN_MAX_PATTERNS", str(1 << 20))
import numpy as np
from phyml_amd import lktree, phyg, synth, workloads


def golden_tree(name):
    """the tree, model and data of tests/golden/<name>.phyg on the device, as the tests make it"""
    from gpu_common import device_tree_from_golden
    d = phyg.load(os.path.join(ROOT, "tests", "golden", name + ".phyg"))
    t, _ = device_tree_from_golden(d)
    return t, np.asarray(d["edge_len"], dtype=np.float64)


def synthetic_tree(n, P, S, seed=7):
    tree = synth.random_tree(n, seed, 0.02, 0.3)
    st = synth.simulate_states(tree, P, S, seed)
    blk = workloads.model_block("model_gtr_g4" if S == 4 else "model_lg_g4")
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, S, int(blk["ncatg"][0]), device=0)
    t.set_model(blk["pi"], blk["gamma_rr"], blk["gamma_r_proba"], blk["e_val"], blk["r_e_vect"], blk["l_e_vect"],
                float(blk["l_min"][0]), float(blk["l_max"][0]), 1.0, 1)
    t.Make_Tree_For_Lk(np.ones(P))
    t.set_tips(tip_states=st.astype(np.int32))
    return t, np.asarray(tree.edge_len, dtype=np.float64)


def one_pass(t, lens, route):
    """route: "device" (asked for), "chain", "rule" (the host layer's own choice).  (seconds of the pass, [(seconds, evaluations)] per
    call, whether every search took the route asked for)"""
    calls, ok = [], True
    t0 = time.perf_counter()
    for e in range(t.ne):
        a = time.perf_counter()
        r = t.Br_Len_Opt(e, force_host_chain=route == "chain", force_device=route == "device")
        calls.append((time.perf_counter() - a, r[3]))
        ok = ok and (route == "rule" or t.on_device == (route == "device"))
        t.edge(e).contents.l = float(lens[e])
        t.Update_PMat_At_Given_Edge(e)
    return time.perf_counter() - t0, calls, ok


def measure(name, t, lens, reps):
    t.Set_Both_Sides(True)
    t.Lk(None)
    row = dict(tree=name, taxa=t.n, patterns=t.P, states=t.S, edges=t.ne)
    for key in ("device", "chain", "rule"):
        _, _, ok = one_pass(t, lens, key)                                      # warm
        if not ok:
            row["device_refused"] = True
            if key == "device":
                continue
        passes = [one_pass(t, lens, key) for _ in range(reps)]
        row[key + "_pass_ms"] = float(np.median([p[0] for p in passes])) * 1e3
        row[key + "_pass_ms_all"] = [p[0] * 1e3 for p in passes]
        ev = np.array([c[1] for c in passes[0][1]])
        # (the routes take the same path per edge -- the tests hold that -- but a pass is classed by its own counts all the same)
        assert all([c[1] for c in p[1]] == list(ev) for p in passes), "evaluation counts changed between repeats"
        per_call = np.median(np.array([[c[0] for c in p[1]] for p in passes]), axis=0) * 1e6
        row[key + "_evaluations"] = int(ev.sum())
        if key == "rule":
            row["rule_on_device"] = bool(t.on_device)
            continue
        for lab, m in (("1-2", ev <= 2), ("3-8", (ev > 2) & (ev <= 8)), (">8", ev > 8)):
            row[f"{key}_us_per_call_{lab}"] = float(per_call[m].mean()) if m.any() else None
            row[f"calls_{lab}"] = int(m.sum())
    if "device_pass_ms" in row:
        t.inst.profile(1)
        t.inst.profile_read_edge_length()
        one_pass(t, lens, "device")
        ms, calls, evals = t.inst.profile_read_edge_length()
        t.inst.profile(0)
        row["kernel_us_per_evaluation"] = ms * 1e3 / max(evals, 1)
        row["kernel_us_per_call"] = ms * 1e3 / max(calls, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    if a.sweep:
        jobs = [("synthetic_nt_24x%d" % P, lambda P=P: synthetic_tree(24, P, 4)) for P in (512, 1024, 4096, 8192, 16384, 32768, 65536, 131072)]
    else:
        jobs = [("nucleic_gtr_g4", lambda: golden_tree("nucleic_gtr_g4")), ("proteic_lg_g4", lambda: golden_tree("proteic_lg_g4")),
                ("synthetic_nt_24x2048", lambda: synthetic_tree(24, 2048, 4)),
                ("synthetic_nt_54x382", lambda: synthetic_tree(54, 382, 4)), ("synthetic_nt_54x256", lambda: synthetic_tree(54, 256, 4))]
    for name, make in jobs:
        t, lens = make()
        try:
            row = measure(name, t, lens, a.reps)
        finally:
            t.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
