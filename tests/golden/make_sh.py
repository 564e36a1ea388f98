#!/usr/bin/env python3
"""Regenerate tests/golden/sh_support_<case>.npz: the inputs and results of the REAL reference's Statistics_To_SH /
Statistics_to_RELL on its own example alignments, and its alias sampler against its own rand() stream, run CPU-only.

Runs only where the reference sources exist and oracle/_ref/libphyml_ref.so has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_sh.py
sh_helper.c (beside this file, this repository's own code) is compiled into a temporary directory against that library; it calls
the reference's public functions in the order of its program entry, then what aLRT() runs in front of its edge loop, then per
internal edge NNI_Neigh_BL, srand(edge), Statistics_To_SH, Statistics_to_RELL.  Each file holds DATA only, every double bit for bit:
    wght [P], init_len, edges [E] (edge numbers), lks [E][3][P] (log_lks_aLRT after NNI_Neigh_BL), sh [E], rell [E],
    seconds [E][2] (what the two statistics took on the machine that generated the file, one host thread),
    alias_w [4][P] (the fixture's weights, all ones, a bootstrap-like vector with zeros, one heavy pattern),
    alias_rand [4][4096] (raw rand() after srand(1)), alias_idx [4][2048] (Sample_n_i_With_Proba_pi(w / init_len, P, 2048) after
    srand(1)), rand_max.
Kept: as many edges as stay within KEEP_BYTES, at least 12 per fixture, spread evenly over the supports in ascending order so that
supports near 0, in between and near 1 are all there (asserted below).
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

REF = os.environ.get("REF", "/root/reference")
REFLIB = os.path.join(ROOT, "oracle", "_ref")
TAIL = ["-c", "4", "-a", "1.0", "-o", "n", "-b", "0"]
CASES = {"nucleic": ("examples_nucleic.phy", ["-d", "nt", "-m", "GTR"]), "proteic": ("examples_proteic.phy", ["-d", "aa", "-m", "LG"])}
KEEP_BYTES = 224 * 1024  # of the three vectors per kept edge, before compression
MIN_EDGES = 12


def parse(txt):
    body = txt[txt.index("SH_BEGIN") + len("SH_BEGIN"):txt.index("SH_END")]
    out = {}
    for line in body.strip().splitlines():
        f = line.split(" ")
        if f[0] == "dims":
            out["dims"] = [int(x) for x in f[2:]]
        else:
            v = np.array([float.fromhex(x) for x in f[2:]])
            assert len(v) == int(f[1]), line[:40]
            out[f[0]] = v
    return out


def main():
    if not os.path.exists(os.path.join(REFLIB, "libphyml_ref.so")) or not os.path.exists(os.path.join(REF, "src", "alrt.c")):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    tmp = tempfile.mkdtemp(prefix="sh_")
    try:
        exe = os.path.join(tmp, "sh_helper")
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-DHAVE_CONFIG_H", "-I" + REF, "-I" + os.path.join(REF, "src"), "-w",
                               os.path.join(HERE, "sh_helper.c"), "-L" + REFLIB, "-lphyml_ref", "-Wl,-rpath," + REFLIB, "-lm", "-o", exe])
        for name, (ali, margs) in CASES.items():
            shutil.copy(os.path.join(HERE, ali), os.path.join(tmp, ali))
            r = subprocess.run([exe, "-i", ali] + margs + TAIL, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0 or "SH_END" not in r.stdout:
                print(r.stdout[-3000:])
                raise SystemExit(f"helper failed: {name}")
            o = parse(r.stdout)
            n, P, init_len = o["dims"]
            edges = sorted(int(k.split("_")[1]) for k in o if k.startswith("stat_"))
            assert len(edges) == n - 3, (len(edges), n)
            stat = {e: o["stat_%d" % e] for e in edges}
            by_sh = sorted(edges, key=lambda e: (stat[e][0], e))
            keep_n = max(MIN_EDGES, min(len(edges), KEEP_BYTES // (3 * P * 8)))
            pick = sorted({by_sh[int(round(i * (len(by_sh) - 1) / (keep_n - 1)))] for i in range(keep_n)})
            sh = np.array([stat[e][0] for e in pick]); rell = np.array([stat[e][1] for e in pick])
            assert len(pick) >= MIN_EDGES, len(pick)
            assert sh.min() <= 0.1 and sh.max() >= 0.9 and ((sh > 0.2) & (sh < 0.8)).any(), sorted(sh)
            d = {"wght": o["wght"], "init_len": np.array([init_len], np.int64), "edges": np.array(pick, np.int32),
                 "lks": np.stack([np.stack([o["lks_%d_%d" % (e, k)] for k in range(3)]) for e in pick]),
                 "sh": sh, "rell": rell, "seconds": np.array([stat[e][2:4] for e in pick]),
                 "alias_w": np.stack([o["alias_w_%d" % v] for v in range(4)]),
                 "alias_rand": np.stack([o["alias_rand_%d" % v] for v in range(4)]).astype(np.int64),
                 "alias_idx": np.stack([o["alias_idx_%d" % v] for v in range(4)]).astype(np.int32),
                 "rand_max": o["rand_max"].astype(np.int64)}
            assert d["wght"].sum() == init_len and d["lks"].shape == (len(pick), 3, P)
            out = os.path.join(HERE, "sh_support_" + name + ".npz")
            np.savez_compressed(out, **d)
            print(f"{name:8s} n={n} P={P} init_len={init_len} edges kept {len(pick)} of {len(edges)}  SH {sh.min():.4f}..{sh.max():.4f}  "
                  f"{np.mean([stat[e][2] for e in edges]):.3f} s per Statistics_To_SH  {os.path.getsize(out) / 1024:.0f} KiB")
            print("   all SH:", " ".join("%.3f" % stat[e][0] for e in by_sh))
            assert os.path.getsize(out) < 512 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
