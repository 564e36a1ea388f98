"""Host time per call of the three candidate-list calls (regraft scan, mixture regraft scan, Triple_Dist) of TWO builds of the library:
the one in phyml_amd/lib ("this") against another directory's ("parent", e.g. the parent commit's build), in fresh child processes
that alternate -- parent, this, this, parent, ... -- because a process settles on one of two levels a few microseconds apart whatever
the build.  Shapes and candidate lists are those of regraft_timing.py, mixture_regraft_timing.py and triple_timing.py (scale 1); only the
call is timed.  Each child reports, per row, REPS medians of CALLS calls after one warm call.  Printed per row: either side's median
and min .. max over all its repeat medians, and whether this build's median lies inside the parent's spread; for K = 1 the
per-process medians as well.
    python tools/scan_overhead.py --parent-lib DIR [--rounds 10] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS, CALLS = 5, 21


def timed(fn):
    import numpy as np
    fn()
    out = []
    for _ in range(REPS):
        ts = []
        for _ in range(CALLS):
            a = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - a)
        out.append(float(np.median(ts)) * 1e6)
    return out


def child():
    import numpy as np
    from phyml_amd import capi
    import regraft_timing as rt
    import mixture_regraft_timing as mt
    import triple_timing as tt
    res = {}
    for shape in ("nt54", "aa37", "nt2048"):
        t, lens = rt.make_tree(shape)
        try:
            t.tree.contents.host_pmat = 0
            t.Set_Both_Sides(True)
            t.Lk(None)
            fn = t.inst.L.phyhip_calculate_regraft_log_likelihoods
            for K in (1, 8, 64, 512):
                cands = rt.candidates(t, lens, K)
                arr = (capi.RegraftCandidate * K)(*[capi.RegraftCandidate(*c) for c in cands])
                out = np.zeros(K)
                res["regraft %s K%d" % (shape, K)] = timed(lambda: capi._chk(fn(t.inst.id, 0, arr, K, -1, capi._ptr(out), None)))
            fn3 = t.inst.L.phyhip_optimise_triples
            inner = list(range(t.n, 2 * t.n - 2))
            for K in (1, 8, 64):
                nodes = [inner[k % len(inner)] for k in range(K)]
                cands = [tt.candidate(t, a, 1.0) for a in nodes]
                arr = (capi.TripleCandidate * K)(*[capi.TripleCandidate((C.c_int * 3)(*x), fl, (C.c_double * 3)(*ln)) for x, fl, ln in cands])
                out3 = (capi.TripleResult * K)()
                res["triple %s K%d" % (shape, K)] = timed(lambda: capi._chk(fn3(t.inst.id, arr, K, capi.BRENT_IT_MAX, C.c_double(1e-3), -1, out3)))
        finally:
            t.close()
    for shape in ("nt4", "lg4x"):
        trees, factors, sums, lens = mt.make_trees(shape)
        try:
            L, n = capi.load(), len(trees)
            ids = (C.c_int * n)(*[t.tree.contents.b_inst for t in trees])
            eig = (C.c_int * n)(*([0] * n))
            da = lambda v: (C.c_double * n)(*[float(x) for x in v])
            proba, rw, ew = da([f[0] for f in factors]), da([f[1] for f in factors]), da([f[2] for f in factors])
            rs, es, sp = (C.c_double(x) for x in sums)
            for K in (1, 8, 64, 512):
                cands = mt.candidates(trees[0], lens, K)
                arr = (capi.RegraftCandidate * K)(*[capi.RegraftCandidate(*c) for c in cands])
                out = np.zeros(K)
                res["mixture %s K%d" % (shape, K)] = timed(lambda: capi._chk(
                    L.phyhip_calculate_mixture_regraft_log_likelihoods(ids, n, eig, arr, K, -1, proba, rw, ew, rs, es, sp, capi._ptr(out), None)))
        finally:
            for t in trees:
                t.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="directory of the other build's libphyhip.so and libphyhip_lk.so")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    import numpy as np
    libs = {"parent": os.path.abspath(a.parent_lib), "this": os.path.join(ROOT, "phyml_amd", "lib")}
    got = {"parent": {}, "this": {}}
    for r in range(a.rounds):
        for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, PHYHIP_LIBDIR=libs[who]),
                               stdout=subprocess.PIPE, text=True, timeout=240)
            if p.returncode != 0:
                print("a run failed (%s, round %d, status %d): nothing more is started" % (who, r, p.returncode), file=sys.stderr)
                return 1
            for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items():
                got[who].setdefault(k, []).extend(v)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(got, open(a.json, "w"), indent=1)
    for k in got["parent"]:
        p, t = got["parent"][k], got["this"][k]
        where = "inside" if min(p) <= np.median(t) <= max(p) else "ABOVE" if np.median(t) > max(p) else "below"
        print("%-22s parent %8.1f [%8.1f .. %8.1f] us   this %8.1f [%8.1f .. %8.1f] us   %s" % (
            k, np.median(p), min(p), max(p), np.median(t), min(t), max(t), where), flush=True)
    for k in got["parent"]:
        if k.endswith("K1"):
            for who in ("parent", "this"):
                v = got[who][k]
                print("%-22s %-6s per process: %s" % (k, who, " ".join("%.1f" % np.median(v[i:i + REPS]) for i in range(0, len(v), REPS))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
