#!/usr/bin/env python3
"""Regenerate tests/golden/pars_<case>.npz: what the REAL reference's parsimony code (src/pars.c) holds after Pars(NULL) with both
sides, in both modes, and what Pars(b) returns at every edge -- run CPU-only.

Runs only where the reference sources exist and oracle/_ref/libphyml_ref.so has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_pars.py
pars_helper.c (beside this file, this repository's own code) is compiled into a temporary directory against that library; it calls the
reference's public functions in the order of its program entry up to Make_Tree_For_Pars (user tree: -u, -o n), then Set_Both_Sides(YES),
Pars(NULL), and Pars(b) for every edge b, for general_pars = NO and YES.  Each file holds DATA only, integers in the smallest dtype:
    n_otu, ns, edge_left / edge_rght [E], node_v / node_b [2n-2][3] (the reference's neighbour order), seq [n_otu][P] (the
    compressed sequences, characters), wght [P], step_mat [ns][ns] (tree->step_mat as the reference filled it at run time),
    ui / pars [E][2][P] (Fitch: left, right side of every edge), site_fitch [E][P], cpars_fitch [E] (Pars(b)),
    site_general [E][P], cpars_general [E], and -- designed cases and the first tree of each example -- ppars [E][2][P][ns].
Cases: examples/nucleic and examples/proteic on their BioNJ tree and on two random topologies (seeded, generated here), and two designed
9-taxon alignments (one per alphabet) that contain every character of the two encoders and constant, fully ambiguous and all-different
columns (the reference's reader rewrites U to T and N ? - to X on the way in, so `seq` holds those as T and X).

    python tests/golden/make_pars.py --time
times Pars(NULL) (both sides) through the helper on one core of this machine at synthetic shapes and prints nanoseconds per
pattern-update: the host baseline of profiles/parsimony.md.
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
TAIL = ["-c", "1", "-o", "n", "-b", "0"]
NT_ARGS, AA_ARGS = ["-d", "nt", "-m", "JC69"], ["-d", "aa", "-m", "LG"]
NT_CHARS, AA_CHARS = "ACGTUMRWSYKBDHVNX?-O", "ARNDCQEGHILKMFPSTWYVBZX?-"


def random_newick(names, seed):
    """a random unrooted binary topology: every next taxon is attached to a random edge"""
    rng = np.random.RandomState(seed)
    order = list(rng.permutation(len(names)))
    # edges as (a, b) over node ids; tips 0..n-1, internal nodes n..
    n = len(names)
    nxt = n
    edges = [(order[0], nxt), (order[1], nxt), (order[2], nxt)]
    nxt += 1
    for t in order[3:]:
        k = rng.randint(len(edges))
        a, b = edges.pop(k)
        edges += [(a, nxt), (nxt, b), (t, nxt)]
        nxt += 1
    adj = {}
    for a, b in edges:
        adj.setdefault(a, []).append(b)
        adj.setdefault(b, []).append(a)

    def sub(node, parent):
        if node < n:
            return "%s:0.1" % names[node]
        return "(" + ",".join(sub(v, node) for v in adj[node] if v != parent) + "):0.1"

    root = n
    return "(" + ",".join(sub(v, root) for v in adj[root]) + ");"


def phylip_names(path):
    lines = [l for l in open(path).read().splitlines() if l.strip()]
    n = int(lines[0].split()[0])
    return [l.split()[0] for l in lines[1:1 + n]]


def designed(chars, seed, ns_plain):
    """9 taxa: every character of the encoder in every taxon at least once, then constant, fully ambiguous and all-different columns"""
    rng = np.random.RandomState(seed)
    n = 9
    cols = []
    for k, c in enumerate(chars):  # a column per character: it sits in taxon k mod 9, unambiguous states elsewhere
        col = [chars[rng.randint(ns_plain)] for _ in range(n)]
        col[k % n] = c
        cols.append(col)
    for _ in range(30):             # random columns over the whole alphabet
        cols.append([chars[rng.randint(len(chars))] for _ in range(n)])
    cols.append([chars[0]] * n)                                 # constant
    cols.append([chars[0]] * n)                                 # ... twice (weight 2 after compaction)
    cols.append([chars[3]] * n)
    amb = [c for c in chars if c in "NX?-O"] if ns_plain == 4 else [c for c in chars if c in "X?-"]
    cols.append([amb[i % len(amb)] for i in range(n)])          # fully ambiguous
    cols.append([c for c in chars if c not in "UN?-O"][:n])       # all different (also after the reader's rewriting)
    cols.append([chars[(i * 2 + 1) % ns_plain] for i in range(n)])
    assert len(cols) < 100
    seqs = ["".join(col[t] for col in cols) for t in range(n)]
    names = ["tax%d" % t for t in range(n)]
    txt = " %d %d\n" % (n, len(cols)) + "".join("%-10s %s\n" % (names[t], seqs[t]) for t in range(n))
    return names, txt


def parse(txt):
    body = txt[txt.index("PARS_BEGIN") + len("PARS_BEGIN"):txt.index("PARS_END")]
    out, times = {}, {}
    for line in body.strip().splitlines():
        f = line.split(" ")
        name, a, b = f[0].rsplit("_", 2)
        if name == "time":
            times[int(a)] = (float(f[2]), float(f[4]))
            continue
        v = np.array(f[2:], dtype=np.int64)
        assert len(v) == int(f[1]), line[:40]
        out[(name, int(a), int(b))] = v
    return out, times


def smallest(a):
    a = np.asarray(a, dtype=np.int64)
    for dt in (np.uint8, np.int8, np.int16, np.int32, np.int64):
        if a.min() >= np.iinfo(dt).min and a.max() <= np.iinfo(dt).max:
            return a.astype(dt)
    raise AssertionError


def run(exe, tmp, ali, margs, newick=None, env=None):
    args = [exe, "-i", ali] + margs + TAIL
    if newick is not None:
        with open(os.path.join(tmp, "user_tree.nwk"), "w") as f:
            f.write(newick + "\n")
        args += ["-u", "user_tree.nwk"]
    r = subprocess.run(args, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if r.returncode != 0 or "PARS_END" not in r.stdout:
        print(r.stdout[-3000:])
        raise SystemExit("helper failed: %s" % ali)
    return parse(r.stdout)


def pack(o, keep_ppars):
    n, P, ns = (int(x) for x in o[("dims", 0, 0)])
    E = 2 * n - 3
    ed = o[("edges", 0, 0)].reshape(E, 2)
    d = {"n_otu": np.array([n], np.int32), "ns": np.array([ns], np.int32), "edge_left": smallest(ed[:, 0]), "edge_rght": smallest(ed[:, 1]),
         "node_v": smallest(o[("node_v", 0, 0)].reshape(2 * n - 2, 3)), "node_b": smallest(o[("node_b", 0, 0)].reshape(2 * n - 2, 3)),
         "seq": np.stack([o[("seq", i, 0)] for i in range(n)]).astype(np.uint8), "wght": smallest(o[("wght", 0, 0)]),
         "step_mat": smallest(o[("step_mat", 0, 0)].reshape(ns, ns)),
         "ui": smallest(np.stack([np.stack([o[("ui", e, s)] for s in (0, 1)]) for e in range(E)])),
         "pars": smallest(np.stack([np.stack([o[("pars", e, s)] for s in (0, 1)]) for e in range(E)])),
         "site_fitch": smallest(np.stack([o[("site", e, 0)] for e in range(E)])),
         "cpars_fitch": smallest(np.array([o[("cpars", e, 0)][0] for e in range(E)])),
         "site_general": smallest(np.stack([o[("site", e, 1)] for e in range(E)])),
         "cpars_general": smallest(np.array([o[("cpars", e, 1)][0] for e in range(E)]))}
    if keep_ppars:
        d["ppars"] = smallest(np.stack([np.stack([o[("ppars", e, s)].reshape(P, ns) for s in (0, 1)]) for e in range(E)]))
    assert d["ui"].shape == (E, 2, P) and d["site_general"].shape == (E, P)
    return d


def build_helper(tmp):
    if not os.path.exists(os.path.join(REFLIB, "libphyml_ref.so")) or not os.path.exists(os.path.join(REF, "src", "pars.c")):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    exe = os.path.join(tmp, "pars_helper")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-DHAVE_CONFIG_H", "-I" + REF, "-I" + os.path.join(REF, "src"), "-w",
                           os.path.join(HERE, "pars_helper.c"), "-L" + REFLIB, "-lphyml_ref", "-Wl,-rpath," + REFLIB, "-lm", "-o", exe])
    return exe


def main():
    tmp = tempfile.mkdtemp(prefix="pars_")
    try:
        exe = build_helper(tmp)
        jobs = []
        for name, ali, margs in (("nucleic", "examples_nucleic.phy", NT_ARGS), ("proteic", "examples_proteic.phy", AA_ARGS)):
            shutil.copy(os.path.join(HERE, ali), os.path.join(tmp, ali))
            names = phylip_names(os.path.join(tmp, ali))
            jobs.append((name + "_bionj", ali, margs, None, True))
            jobs.append((name + "_random1", ali, margs, random_newick(names, 101), False))
            jobs.append((name + "_random2", ali, margs, random_newick(names, 202), False))
        for name, chars, margs, plain, seed in (("designed_nt", NT_CHARS, NT_ARGS, 4, 7), ("designed_aa", AA_CHARS, AA_ARGS, 20, 8)):
            names, txt = designed(chars, seed, plain)
            with open(os.path.join(tmp, name + ".phy"), "w") as f:
                f.write(txt)
            jobs.append((name, name + ".phy", margs, random_newick(names, seed), True))
        for case, ali, margs, newick, keep in jobs:
            o, _ = run(exe, tmp, ali, margs, newick)
            d = pack(o, keep)
            out = os.path.join(HERE, "pars_" + case + ".npz")
            np.savez_compressed(out, **d)
            size = os.path.getsize(out)
            print(f"{case:16s} n={int(d['n_otu'][0])} P={d['ui'].shape[2]} ns={int(d['ns'][0])} c_pars fitch {int(d['cpars_fitch'][0])} "
                  f"general {int(d['cpars_general'][0])}  {size / 1024:.0f} KiB")
            assert size < 1000 * 1000, size
            if case.startswith("designed"):
                chars = NT_CHARS if d["ns"][0] == 4 else AA_CHARS
                assert int(d["n_otu"][0]) == 9 and d["ui"].shape[2] < 100
                # (the reference's reader rewrites U to T and N ? - to X before the encoders see them: the file has them all, c_seq the rest)
                lost = set(chars) - set(chr(c) for c in d["seq"].ravel())
                assert lost <= set("UN?-"), lost
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_main():
    """Pars(NULL), both sides, through the helper on one core: ns per pattern-update at synthetic shapes"""
    # (cfg5, 500 x 100 000, is cut to 500 x 20 000: the reference allocates ns ints per pattern for every edge side in either mode)
    shapes = [("nt", 54, 382), ("nt", 100, 50000), ("aa", 200, 10000), ("nt", 150, 20000), ("nt", 500, 20000)]
    cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1]
    print("CPU:", cpu[0] if cpu else "unknown")
    tmp = tempfile.mkdtemp(prefix="pars_time_")
    try:
        exe = build_helper(tmp)
        for kind, n, sites in shapes:
            rng = np.random.RandomState(n + sites)
            chars = "ACGT" if kind == "nt" else AA_CHARS[:20]
            names = ["t%d" % i for i in range(n)]
            # columns are drawn independently: nearly every one is a pattern of its own
            seqs = rng.randint(len(chars), size=(n, sites))
            with open(os.path.join(tmp, "time.phy"), "w") as f:
                f.write(" %d %d\n" % (n, sites))
                for i in range(n):
                    f.write("%-10s %s\n" % (names[i], "".join(chars[c] for c in seqs[i])))
            reps = max(1, int(2e8 / (3.0 * n * sites)))
            env = dict(os.environ, PARS_HELPER_TIME=str(reps))
            o, times = run(exe, tmp, "time.phy", NT_ARGS if kind == "nt" else AA_ARGS, random_newick(names, 5), env=env)
            P = int(o[("dims", 0, 0)][1])
            print(f"{kind} {n} x {sites} ({P} patterns, {reps} repeats): Fitch {times[0][0]:.3f} ns per pattern-update, {times[0][1] * 1e3:.3f} ms per "
                  f"Pars(NULL); step matrix {times[1][0]:.3f} ns, {times[1][1] * 1e3:.3f} ms")
            sys.stdout.flush()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    time_main() if "--time" in sys.argv[1:] else main()
