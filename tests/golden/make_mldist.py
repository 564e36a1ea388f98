#!/usr/bin/env python3
"""Regenerate tests/golden/mldist_<case>.npz: ML_Dist of the REAL reference with its own starting values, run CPU-only.

Runs only where the reference sources exist and oracle/_ref/libphyml_ref.so has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_mldist.py
mldist_helper.c (beside this file, this repository's own code) is compiled into a temporary directory against that library; it
calls the reference's public functions in the order of its program entry, then K80_dist / JC69_Dist, then ML_Dist.  Each file
holds DATA only, every double bit for bit: the compacted characters [n][P], wght, pi, e_val, r_e_vect, l_e_vect, l_min, l_max,
min_diff_lk_local, the reference's starting matrix and its ML_Dist matrix; the designed cases also the pairs that take each rare
branch (asserted here on the reference's own output before the file is written).

Cases: the two example alignments, and one designed alignment per alphabet (12 taxa x 60 sites) holding
    (0, 1)  two identical sequences                                  -> d = l_min
    (2, 3)  no common unambiguous site                               -> start = -1, sum F < .001, d = 0.1
    (0, 4)  every site a transversion / a mismatch                   -> the closed form is invalid (-1 -> 0.1), the optimum is cut at DIST_MAX
    (0, 5)  a valid closed form above DIST_MAX - SMALL               -> start = DIST_MAX -> 0.1
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
from phyml_amd import synth  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
REFLIB = os.path.join(ROOT, "oracle", "_ref")
TAIL = ["-c", "4", "-a", "1.0", "-o", "n", "-b", "0"]
NT = ["-d", "nt", "-m", "GTR", "-f", "0.3,0.2,0.2,0.3"]
AA = ["-d", "aa", "-m", "LG", "-f", "m"]
BRANCH_PAIRS = {"identical": (0, 1), "disjoint": (2, 3), "saturated": (0, 4), "over": (0, 5)}


def designed(ns, seed):
    """[12][60] characters (see the module docstring)."""
    n, L = 12, 60
    alpha = np.frombuffer((synth.NT_ALPHABET if ns == 4 else synth.AA_ALPHABET).encode(), dtype=np.uint8)
    h = lambda stream, size: synth.hash_u64(seed, stream, np.arange(size))
    base = (h(1, L) % np.uint64(ns)).astype(np.int64)
    st = np.zeros((n, L), np.int64)
    st[0] = base
    st[1] = base
    st[2] = (h(2, L) % np.uint64(ns)).astype(np.int64)
    st[3] = (h(3, L) % np.uint64(ns)).astype(np.int64)
    if ns == 4:
        st[4] = base ^ 1                      # A <-> C, G <-> T: a transversion at every site
        st[5] = base.copy()
        st[5][:17] = base[:17] ^ 2            # 17 transitions (A <-> G, C <-> T)
        st[5][17:41] = base[17:41] ^ 1        # 24 transversions: 1 - 2P - Q = 2/60, K80 = 2.1
    else:
        st[4] = (base + 1) % ns               # a mismatch at every site
        st[5] = base.copy()
        st[5][:54] = (base[:54] + 3) % ns     # P = 54/60: JC69 = 2.8
    for t in range(6, n):
        hit = (h(10 + t, L) % np.uint64(100)).astype(np.int64) < 8 * (t - 4)
        new = (h(30 + t, L) % np.uint64(ns)).astype(np.int64)
        st[t] = np.where(hit, new, base)
    chars = alpha[st]
    chars[2, L // 2:] = ord("-")
    chars[3, :L // 2] = ord("-")
    amb = np.frombuffer(b"RYN-" if ns == 4 else b"X-", dtype=np.uint8)
    for t in range(6, n):
        idx = np.arange(t % 7, L, 7)
        chars[t, idx] = amb[(idx + t) % len(amb)]
    return chars


def parse(txt):
    body = txt[txt.index("MLDIST_BEGIN") + len("MLDIST_BEGIN"):txt.index("MLDIST_END")]
    out, chars = {}, {}
    for line in body.strip().splitlines():
        f = line.split(" ")
        if f[0] == "chars":
            chars[int(f[1])] = np.frombuffer(f[2].encode(), dtype=np.uint8)
        elif f[0] == "dims":
            out["dims"] = [int(x) for x in f[2:]]
        else:
            v = np.array([float.fromhex(x) for x in f[2:]])
            assert len(v) == int(f[1]), line[:40]
            out[f[0]] = v
    n, P, S = out.pop("dims")
    d = {"chars": np.stack([chars[t] for t in range(n)])}
    assert d["chars"].shape == (n, P)
    for k in ("wght", "pi", "e_val", "l_min", "l_max", "min_diff_lk_local"):
        d[k] = out[k]
    d["r_e_vect"] = out["r_e_vect"].reshape(S, S)
    d["l_e_vect"] = out["l_e_vect"].reshape(S, S)
    d["start"] = np.stack([out["start_%d" % j] for j in range(n)])
    d["dist"] = np.stack([out["dist_%d" % j] for j in range(n)])
    return d


def main():
    if not os.path.exists(os.path.join(REFLIB, "libphyml_ref.so")) or not os.path.exists(os.path.join(REF, "src", "lk.c")):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    tmp = tempfile.mkdtemp(prefix="mldist_")
    try:
        exe = os.path.join(tmp, "mldist_helper")
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-DHAVE_CONFIG_H", "-I" + REF, "-I" + os.path.join(REF, "src"), "-w",
                               os.path.join(HERE, "mldist_helper.c"), "-L" + REFLIB, "-lphyml_ref", "-Wl,-rpath," + REFLIB, "-lm", "-o", exe])
        cases, ns_of = {}, {"designed_nt": 4, "designed_aa": 20}
        for name, src, margs in (("nucleic", "examples_nucleic.phy", NT), ("proteic", "examples_proteic.phy", AA)):
            shutil.copy(os.path.join(HERE, src), os.path.join(tmp, src))
            cases[name] = (src, margs)
        for name, ns, margs in (("designed_nt", 4, NT), ("designed_aa", 20, AA)):
            # (the reference orders the taxa by name, last first: named so that taxon t is row t of its compacted data)
            synth.write_phylip(os.path.join(tmp, name + ".phy"), ["T%02d" % (11 - i) for i in range(12)], designed(ns, 41 + ns))
            cases[name] = (name + ".phy", margs)
        for name, (ali, margs) in cases.items():
            r = subprocess.run([exe, "-i", ali] + margs + TAIL, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0 or "MLDIST_END" not in r.stdout:
                print(r.stdout[-3000:])
                raise SystemExit(f"helper failed: {name}")
            d = parse(r.stdout)
            D, S0 = d["dist"], d["start"]
            assert np.array_equal(D, D.T) and not D.diagonal().any()
            if name.startswith("designed"):
                l_min = d["l_min"][0]
                want = designed(4 if name.endswith("nt") else 20, 41 + (4 if name.endswith("nt") else 20))
                gap = lambda c: np.where(np.isin(c, [ord("X"), ord("N")] if ns_of[name] == 4 else [ord("X")]), ord("-"), c)  # (the reader's spelling of "any state")
                assert d["chars"].shape[1] == 60 and np.array_equal(gap(d["chars"]), gap(want)), name
                (a, b), (c, e), (f, g), (h, i) = (BRANCH_PAIRS[k] for k in ("identical", "disjoint", "saturated", "over"))
                assert np.array_equal(d["chars"][a], d["chars"][b]) and D[a, b] == l_min, (name, D[a, b])
                assert S0[c, e] == -1.0 and D[c, e] == 0.1, (name, S0[c, e], D[c, e])
                assert S0[f, g] == -1.0 and D[f, g] == 2.0, (name, S0[f, g], D[f, g])
                assert S0[h, i] == 2.0, (name, S0[h, i])
                for k, v in BRANCH_PAIRS.items():
                    d["pair_" + k] = np.array(v, dtype=np.int32)
            out = os.path.join(HERE, "mldist_" + name + ".npz")
            np.savez_compressed(out, **d)
            print(f"{name:12s} n={D.shape[0]} P={d['chars'].shape[1]} max d={D.max():.4f}  {os.path.getsize(out) / 1024:.0f} KiB")
            assert os.path.getsize(out) < 100 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
