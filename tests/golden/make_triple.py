#!/usr/bin/env python3
"""Regenerate tests/golden/triple_<case>.npz: what the REAL reference's Triple_Dist (src/utilities.c:7120-7146) does at every internal
node of the trees the committed .phyg files describe, from the committed lengths and with the node's three edges scaled by 0.05 and
by 20, run CPU-only.

Runs only where the reference sources exist and oracle/_ref/libphyml_ref.so has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_triple.py
triple_helper.c (beside this file, this repository's own code) is compiled into a temporary directory against that library and run
with make_golden.py's command lines for the three cases.  Per record the reference gives scalars only: node, scaling, the three
lengths out, c_lnL and the growth of tree->n_tot_bl_opt.

Thin decisions are removed HERE, on the CPU, by make_brlen.py's rule applied to each of the record's three searches: the restatement of
tests/triple_ref.py is driven over the CPU oracle on the tree of the .phyg, and a record is dropped when any decision of any of its
searches lies within 64 bounds of flipping (B_lnl, B_dlnl = P * 2^-52 * sum |terms| over that search's probes; roots: 64 x
root_spread).  At every kept record the restatement must reproduce the reference's n_tot_bl_opt growth.  The script prints how many it
dropped and fails if that is more than one in ten of a case.  Every committed record is then compared by the tests; none is skipped
there.

Each file holds DATA only, every double bit for bit:
    node, scale [R], edges [R][3], l_in, l_out [R][3], lnL [R], n_tot [R]                             -- the reference's
    evaluations, status, best_from [R][3] (0 start, 1 geometric, 2 spline)                             -- the paths, from the restatement
    l_min, l_max, tol, iter_max, edge_len [E], scales, dropped [D][2] (node, scaling index of the records removed)
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_brlen import BEST_FROM, CASES, REF, REFLIB, thin  # noqa: E402  (the cases' command lines and the 64 x bound rule)

SCALES = (1.0, 0.05, 20.0)


def parse(txt):
    body = txt[txt.index("TRIPLE_BEGIN") + len("TRIPLE_BEGIN"):txt.index("TRIPLE_END")]
    out = {"rec": []}
    for line in body.strip().splitlines():
        f = line.split(" ")
        if f[0] == "dims":
            out["dims"] = [int(x) for x in f[1:]]
        elif f[0] == "opt":
            out["opt"] = [float.fromhex(x) for x in f[1:4]] + [int(f[4])]
        elif f[0] == "edge_len":
            out["edge_len"] = np.array([float.fromhex(x) for x in f[1:]])
        elif f[0] == "rec":
            out["rec"].append((int(f[1]), int(f[2]), [int(x) for x in f[3:6]], [float.fromhex(x) for x in f[6:9]],
                               [float.fromhex(x) for x in f[9:12]], float.fromhex(f[12]), int(f[13])))
    return out


def main():
    if not os.path.exists(os.path.join(REFLIB, "libphyml_ref.so")) or not os.path.exists(os.path.join(REF, "src", "utilities.c")):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    import orc
    import phyg
    import triple_ref
    tmp = tempfile.mkdtemp(prefix="triple_")
    try:
        exe = os.path.join(tmp, "triple_helper")
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-DHAVE_CONFIG_H", "-I" + REF, "-I" + os.path.join(REF, "src"), "-w",
                               os.path.join(HERE, "triple_helper.c"), "-L" + REFLIB, "-lphyml_ref", "-Wl,-rpath," + REFLIB, "-lm", "-o", exe])
        for ali in ("examples_nucleic.phy", "examples_proteic.phy"):
            shutil.copy(os.path.join(HERE, ali), os.path.join(tmp, ali))
        for name, (hopts, margs) in CASES.items():
            r = subprocess.run([exe] + hopts + ["--"] + margs, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0 or "TRIPLE_END" not in r.stdout:
                print(r.stdout[-3000:])
                raise SystemExit(f"helper failed: {name}")
            o = parse(r.stdout)
            n, P, E = o["dims"]
            l_min, l_max, tol, iter_max = o["opt"]
            d = phyg.load(os.path.join(HERE, name + ".phyg"))
            assert np.array_equal(o["edge_len"], d["edge_len"]) and P == len(d["wght"]), name  # the tree of the .phyg, to the bits
            ot = orc.tree_from_golden(d)
            ot.lk(None, both_sides=True)
            assert ot.m.l_min == l_min and ot.m.l_max == l_max
            keep, dropped, worst_l, worst_lnl = [], [], 0.0, 0.0
            for (a, k, edges, l_in, l_out, c_lnl, n_tot) in o["rec"]:
                assert triple_ref.edges_of(ot, a) == edges, (name, a)               # a->b[0..2] of the .phyg are the reference's
                l0 = [float(d["edge_len"][e]) for e in edges]
                assert l_in == [min(x * SCALES[k], 90.0) for x in l0], (name, a, k)
                for e, l in zip(edges, l_in):
                    ot.len[e] = l
                flags = []

                def after(i, s):
                    b_lnl = b_dlnl = 0.0
                    for (lc, _, _) in s.result.probes:
                        _, x, y = ot.dlk_terms(lc)
                        b_lnl = max(b_lnl, ot.P * 2.0 ** -52 * float(np.abs(x).sum()))
                        b_dlnl = max(b_dlnl, ot.P * 2.0 ** -52 * float(np.abs(y).sum()))
                    flags.append(thin(s.result, b_lnl, b_dlnl)[0] or abs(s.result.lnL - (s.lk_begin - tol)) < 64.0 * b_lnl)
                t = triple_ref.triple_dist(ot, a, iter_max, tol, after)
                triple_ref.restore(ot, edges, l0)
                for e in edges:
                    ot.update_partial(e, a)
                if any(flags):
                    dropped.append((a, k))
                    continue
                # a kept record's path is the reference's: the same steps, and statuses the reference returns from
                assert t.n_tot == n_tot and all(s.status in (0, 1, 2) for s in t.searches) and len(t.searches) == 3, (name, a, k, t.n_tot, n_tot)
                for got, want in zip(t.lengths, l_out):
                    worst_l = max(worst_l, abs(got - want) / max(abs(want), 1e-300))
                worst_lnl = max(worst_lnl, abs(t.lnL - c_lnl) / abs(c_lnl))
                keep.append((a, k, edges, l_in, l_out, c_lnl, n_tot, [s.result.evaluations for s in t.searches], [s.status for s in t.searches],
                             [BEST_FROM[s.result.best_from] for s in t.searches]))
            total = len(o["rec"])
            print(f"{name:20s} n={n} P={P} records {total} dropped {len(dropped)} ({100.0 * len(dropped) / total:.1f} %)  "
                  f"largest relative difference restatement vs reference: l_out {worst_l:.3e}  c_lnL {worst_lnl:.3e}")
            if len(dropped) * 10 > total:
                raise SystemExit(f"{name}: more than one record in ten has a thin decision")
            c = list(zip(*keep))
            out = os.path.join(HERE, "triple_" + name + ".npz")
            np.savez_compressed(out, node=np.array(c[0], np.int32), scale=np.array([SCALES[k] for k in c[1]]), edges=np.array(c[2], np.int32),
                                l_in=np.array(c[3]), l_out=np.array(c[4]), lnL=np.array(c[5]), n_tot=np.array(c[6], np.int32),
                                evaluations=np.array(c[7], np.int32), status=np.array(c[8], np.int32), best_from=np.array(c[9], np.int32),
                                l_min=np.array([l_min]), l_max=np.array([l_max]), tol=np.array([tol]), iter_max=np.array([iter_max], np.int32),
                                edge_len=o["edge_len"], scales=np.array(SCALES), dropped=np.array(dropped, np.int32).reshape(-1, 2))
            ev = np.array(c[7])
            print(f"   kept {len(keep)}: evaluations per search min {ev.min()} max {ev.max()}  status 0/1/2: "
                  f"{[int((np.array(c[8]) == s).sum()) for s in (0, 1, 2)]}  {os.path.getsize(out) / 1024:.0f} KiB")
            assert os.path.getsize(out) < 256 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
