#!/usr/bin/env python3
"""Regenerate tests/golden/brlen_<case>.npz: what the REAL reference's Br_Len_Opt (src/optimiz.c:607-663, with its static
Br_Len_Spline, :2244-2470) does on every edge of the trees the committed .phyg files describe, from six start lengths per edge, run
CPU-only.

Runs only where the reference sources exist and oracle/_ref/libphyml_ref.so has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_brlen.py
brlen_helper.c (beside this file, this repository's own code) is compiled into a temporary directory against that library and run
with make_golden.py's command lines for the three cases.  Per record the reference gives scalars only: edge, l_in, lk_begin,
l_out, c_lnL, c_dlnL and the growth of tree->n_tot_bl_opt.

Thin decisions are removed HERE, on the CPU and with the reference's records alone.  The restatement of tests/brlen_ref.py is driven
over the CPU oracle on the tree of the .phyg; it must reproduce the reference's n_tot_bl_opt growth at every record, and it names
every decision the path took with its margin.  With B = P * 2^-52 * sum |terms| -- the summation bound the SH tests use -- taken
over the per-pattern lnL terms (B_lnl) and dlnL terms (B_dlnl) at every probe of the record, a record is dropped when
    a sign test saw |dlnL| < 64 B_dlnl,  a best-so-far or convergence test came within 64 B_lnl,
    or the accepted root came within 64 x root_spread(B_lnl, B_dlnl) of u, v, the other root or the 1e-5 bands:
another summation order could send such a search down another path.  The script prints how many it dropped and fails if that is
more than one in ten of a case.  Every committed record is then compared by the tests; none is skipped there.

Each file holds DATA only, every double bit for bit:
    edge, start [R] (index into FACTORS), l_in, lk_begin, l_out, c_lnL, c_dlnL [R], n_tot [R]      -- the reference's
    evaluations, status [R], best_from [R] (0 start, 1 geometric, 2 spline)                           -- the path, from the restatement
    b_lnl, b_dlnl [R] (the two bounds, largest over the record's probes), root_spread [R] (0 where no spline step)
    l_min, l_max, tol, iter_max, edge_len [E], dropped [D][2] (edge, start of the records removed)
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

REF = os.environ.get("REF", "/root/reference")
REFLIB = os.path.join(ROOT, "oracle", "_ref")
GTR_RR = "1,2.5,0.8,1.2,3.0,1"
NT_FREQ = "0.3,0.2,0.2,0.3"
FACTORS = (1.0, 0.05, 20.0, 1e-6, 1e3, -1.0)
# (helper options, phyml command line): tests/golden/make_golden.py's, the alignment under its committed name
CASES = {
    "nucleic_gtr_g4": ([], ["-i", "examples_nucleic.phy", "-d", "nt", "-m", "GTR", "-c", "4", "-a", "1.0", "-o", "n", "-b", "0"]),
    "nucleic_gtr_g4_inv": (["--gtr-rr", GTR_RR], ["-i", "examples_nucleic.phy", "-d", "nt", "-m", "GTR", "-f", NT_FREQ, "-c", "4", "-a", "0.7",
                                                   "-v", "0.2", "-o", "n", "-b", "0"]),
    "proteic_lg_g4": ([], ["-i", "examples_proteic.phy", "-d", "aa", "-m", "LG", "-c", "4", "-a", "1.0", "-o", "n", "-b", "0"]),
}
BEST_FROM = {"start": 0, "geometric": 1, "spline": 2}


def parse(txt):
    body = txt[txt.index("BRLEN_BEGIN") + len("BRLEN_BEGIN"):txt.index("BRLEN_END")]
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
            out["rec"].append((int(f[1]), int(f[2])) + tuple(float.fromhex(x) for x in f[3:8]) + (int(f[8]),))
    return out


def replay(ot, e, l_in, l0, l_min, l_max, iter_max, tol):
    """the restatement over the oracle for one record: (Result, lk_begin, B_lnl, B_dlnl)"""
    import brlen_ref
    ot.len[e] = l_in
    lk_begin = ot.lk(e)
    ot.update_eigen_lr(e)
    r = brlen_ref.br_len_spline(ot.dlk, l_in, lk_begin, l_min, l_max, iter_max, tol)
    b_lnl = b_dlnl = 0.0
    for (lc, _, _) in r.probes:
        _, a, b = ot.dlk_terms(lc)
        b_lnl = max(b_lnl, ot.P * 2.0 ** -52 * float(np.abs(a).sum()))
        b_dlnl = max(b_dlnl, ot.P * 2.0 ** -52 * float(np.abs(b).sum()))
    ot.len[e] = l0
    ot.update_pmat(e)
    return r, lk_begin, b_lnl, b_dlnl


def thin(r, b_lnl, b_dlnl):
    """whether a decision of the path lies within 64 bounds of flipping, and the spread of the accepted root"""
    import brlen_ref
    spread = brlen_ref.root_spread(r.spline, b_lnl, b_dlnl) if r.spline is not None else 0.0
    for kind, margin in r.decisions:
        bound = {"sign": b_dlnl, "best": b_lnl, "tol": b_lnl, "root": spread}[kind]
        if margin < 64.0 * bound:
            return True, spread
    return False, spread


def main():
    if not os.path.exists(os.path.join(REFLIB, "libphyml_ref.so")) or not os.path.exists(os.path.join(REF, "src", "optimiz.c")):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    import orc
    import phyg
    tmp = tempfile.mkdtemp(prefix="brlen_")
    try:
        exe = os.path.join(tmp, "brlen_helper")
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-DHAVE_CONFIG_H", "-I" + REF, "-I" + os.path.join(REF, "src"), "-w",
                               os.path.join(HERE, "brlen_helper.c"), "-L" + REFLIB, "-lphyml_ref", "-Wl,-rpath," + REFLIB, "-lm", "-o", exe])
        for ali in ("examples_nucleic.phy", "examples_proteic.phy"):
            shutil.copy(os.path.join(HERE, ali), os.path.join(tmp, ali))
        for name, (hopts, margs) in CASES.items():
            r = subprocess.run([exe] + hopts + ["--"] + margs, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0 or "BRLEN_END" not in r.stdout:
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
            keep, dropped, worst = [], [], 0.0
            for (e, k, l_in, lk_begin, l_out, c_lnl, c_dlnl, n_tot) in o["rec"]:
                res, lkb, b_lnl, b_dlnl = replay(ot, e, l_in, float(d["edge_len"][e]), l_min, l_max, iter_max, tol)
                is_thin, spread = thin(res, b_lnl, b_dlnl)
                if is_thin:
                    dropped.append((e, k))
                    continue
                # a kept record's path is the reference's: the same steps, and a status the reference returns from
                assert res.n_tot == n_tot and res.status in (0, 1, 2), (name, e, k, res.n_tot, n_tot, res.status)
                assert res.evaluations == n_tot + (0 if res.status in (1, 2) else 1)
                for a, b in ((lkb, lk_begin), (res.l, l_out), (res.lnL, c_lnl), (res.dlnL, c_dlnl)):
                    if a != b:
                        worst = max(worst, abs(a - b) / max(abs(b), 1e-300))
                keep.append((e, k, l_in, lk_begin, l_out, c_lnl, c_dlnl, n_tot, res.evaluations, res.status, BEST_FROM[res.best_from],
                             b_lnl, b_dlnl, spread))
            total = len(o["rec"])
            print(f"{name:20s} n={n} P={P} records {total} dropped {len(dropped)} ({100.0 * len(dropped) / total:.1f} %)  "
                  f"largest relative difference oracle vs reference over lk_begin, l_out, c_lnL, c_dlnL: {worst:.3e}")
            if len(dropped) * 10 > total:
                raise SystemExit(f"{name}: more than one record in ten has a thin decision")
            c = list(zip(*keep))
            out = os.path.join(HERE, "brlen_" + name + ".npz")
            np.savez_compressed(out, edge=np.array(c[0], np.int32), start=np.array(c[1], np.int32), l_in=np.array(c[2]), lk_begin=np.array(c[3]),
                                l_out=np.array(c[4]), c_lnL=np.array(c[5]), c_dlnL=np.array(c[6]), n_tot=np.array(c[7], np.int32),
                                evaluations=np.array(c[8], np.int32), status=np.array(c[9], np.int32), best_from=np.array(c[10], np.int32),
                                b_lnl=np.array(c[11]), b_dlnl=np.array(c[12]), root_spread=np.array(c[13]),
                                l_min=np.array([l_min]), l_max=np.array([l_max]), tol=np.array([tol]), iter_max=np.array([iter_max], np.int32),
                                edge_len=o["edge_len"], factors=np.array(FACTORS), dropped=np.array(dropped, np.int32).reshape(-1, 2))
            ev = np.array(c[8])
            print(f"   kept {len(keep)}: evaluations 1-2: {(ev <= 2).sum()}  3-8: {((ev > 2) & (ev <= 8)).sum()}  > 8: {(ev > 8).sum()}  max {ev.max()}  "
                  f"status 0/1/2: {[int((np.array(c[9]) == s).sum()) for s in (0, 1, 2)]}  {os.path.getsize(out) / 1024:.0f} KiB")
            assert os.path.getsize(out) < 256 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
