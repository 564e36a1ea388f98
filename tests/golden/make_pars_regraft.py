#!/usr/bin/env python3
"""Regenerate tests/golden/regraft_pars_<case>.npz: what the REAL reference's parsimony code returns for the candidates of the
parsimony SPR scan (Test_One_Spr_Target under spr_pars, src/spr.c:639-651), in both modes -- run CPU-only.

Runs only where the reference sources exist and oracle/_ref/libphyml_ref.so has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_pars_regraft.py
pars_regraft_helper.c (beside this file, this repository's own code) is compiled into a temporary directory against that library.  For
a prune site (edge b, link node) it prunes with the reference's Prune_Subtree and, for EVERY edge t of the residual tree, grafts the
subtree onto t, runs Pars(NULL) with both sides on the grafted tree and Pars(b), and prunes again -- for general_pars = NO and YES.
Each file holds DATA only, integers in the smallest dtype, in the numbering of pars_<case>.npz (same alignments, same trees, same
seeds -- make_pars.py's own generators are imported; the topology the helper built is asserted equal to that file's):
    prune [K][3]: edge, link node, the node on the other end (the root of the pruned subtree);
    target_off [K + 1]: site k's candidates are rows target_off[k] .. target_off[k + 1] of
    target_edge [T], target_ends [T][2] (the target edge's two end nodes in the PRUNED tree), c_pars_fitch [T], c_pars_general [T]
    and -- designed cases -- site_fitch [T][P], site_general [T][P].
(The files are not called pars_regraft_<case>.npz: tests/test_parsimony_restatement.py takes every pars_*.npz for a fixture of its own.)
Cases: the two designed 9-taxon alignments on the tree make_pars.py gives them -- every prune site in both directions, every target,
site_pars kept -- and examples/nucleic and examples/proteic on their BioNJ tree: six prune sites drawn with a fixed seed (one of them
forced to have a tip as the subtree), every target, c_pars only.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_pars as mp  # noqa: E402  (the generators of pars_<case>.npz: alignments, trees, seeds)


def build_helper(tmp):
    import subprocess
    if not os.path.exists(os.path.join(mp.REFLIB, "libphyml_ref.so")) or not os.path.exists(os.path.join(mp.REF, "src", "pars.c")):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    exe = os.path.join(tmp, "pars_regraft_helper")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-DHAVE_CONFIG_H", "-I" + mp.REF, "-I" + os.path.join(mp.REF, "src"), "-w",
                           os.path.join(HERE, "pars_regraft_helper.c"), "-L" + mp.REFLIB, "-lphyml_ref", "-Wl,-rpath," + mp.REFLIB, "-lm",
                           "-o", exe])
    return exe


def draw_sites(base, seed, count=6):
    """`count` prune sites (edge, link) of the fixture's tree, drawn with a fixed seed; at least one has a tip as the subtree"""
    n = int(base["n_otu"][0])
    left, rght = [int(x) for x in base["edge_left"]], [int(x) for x in base["edge_rght"]]
    sites = [(e, x) for e in range(len(left)) for x in (left[e], rght[e]) if x >= n]
    other = lambda s: rght[s[0]] if s[1] == left[s[0]] else left[s[0]]
    order = [sites[i] for i in np.random.RandomState(seed).permutation(len(sites))]
    pick = order[:count]
    if not any(other(s) < n for s in pick):
        pick[-1] = next(s for s in order if other(s) < n)
    assert any(other(s) < n for s in pick) and any(other(s) >= n for s in pick)
    return pick


def pack(o, base, keep_site):
    n, P, ns, K = (int(x) for x in o[("dims", 0, 0)])
    E = 2 * n - 3
    ed = o[("edges", 0, 0)].reshape(E, 2)
    assert n == int(base["n_otu"][0]) and ns == int(base["ns"][0]) and P == base["wght"].shape[0]
    assert np.array_equal(ed[:, 0], base["edge_left"]) and np.array_equal(ed[:, 1], base["edge_rght"]), "not the tree of pars_<case>.npz"
    prune, off, tgt, cf, cg, sf, sg = [], [0], [], [], [], [], []
    for k in range(K):
        prune.append(o[("prune", k, 0)])
        nt = int(o[("ntargets", k, 0)][0])
        for j in range(nt):
            tgt.append(o[("target", k, j)])
            cf.append(o[("cp", k * 1000 + j, 0)][0]); cg.append(o[("cp", k * 1000 + j, 1)][0])
            if keep_site:
                sf.append(o[("sp", k * 1000 + j, 0)]); sg.append(o[("sp", k * 1000 + j, 1)])
        off.append(len(tgt))
    tgt = np.array(tgt)
    d = {"prune": mp.smallest(np.array(prune)), "target_off": mp.smallest(np.array(off)), "target_edge": mp.smallest(tgt[:, 0]),
         "target_ends": mp.smallest(tgt[:, 1:3]), "c_pars_fitch": mp.smallest(np.array(cf)), "c_pars_general": mp.smallest(np.array(cg))}
    if keep_site:
        d["site_fitch"] = mp.smallest(np.stack(sf)); d["site_general"] = mp.smallest(np.stack(sg))
        assert d["site_fitch"].shape == (len(tgt), P)
    return d


def main():
    tmp = tempfile.mkdtemp(prefix="pars_regraft_")
    try:
        exe = build_helper(tmp)
        jobs = []
        for name, chars, margs, plain, seed in (("designed_nt", mp.NT_CHARS, mp.NT_ARGS, 4, 7), ("designed_aa", mp.AA_CHARS, mp.AA_ARGS, 20, 8)):
            names, txt = mp.designed(chars, seed, plain)
            with open(os.path.join(tmp, name + ".phy"), "w") as f:
                f.write(txt)
            jobs.append((name, name + ".phy", margs, mp.random_newick(names, seed), "all", True))
        for name, ali, margs, seed in (("nucleic_bionj", "examples_nucleic.phy", mp.NT_ARGS, 31), ("proteic_bionj", "examples_proteic.phy", mp.AA_ARGS, 32)):
            shutil.copy(os.path.join(HERE, ali), os.path.join(tmp, ali))
            base = np.load(os.path.join(HERE, "pars_" + name + ".npz"))
            jobs.append((name, ali, margs, None, ",".join("%d:%d" % s for s in draw_sites(base, seed)), False))
        for case, ali, margs, newick, sites, keep in jobs:
            base = np.load(os.path.join(HERE, "pars_" + case + ".npz"))
            env = dict(os.environ, PARS_REGRAFT_SITES=sites, PARS_REGRAFT_KEEP_SITE="1" if keep else "0")
            o, _ = mp.run(exe, tmp, ali, margs, newick, env=env)
            d = pack(o, base, keep)
            n = int(base["n_otu"][0])
            if not keep:   # a tip as the subtree, and a tip at an end of a target edge
                assert (d["prune"][:, 2] < n).any() and (d["target_ends"] < n).any()
            out = os.path.join(HERE, "regraft_pars_" + case + ".npz")
            np.savez_compressed(out, **d)
            size = os.path.getsize(out)
            print(f"{case:16s} sites={d['prune'].shape[0]} candidates={d['target_edge'].shape[0]} c_pars fitch {int(d['c_pars_fitch'].min())}.."
                  f"{int(d['c_pars_fitch'].max())} general {int(d['c_pars_general'].min())}..{int(d['c_pars_general'].max())}  {size / 1024:.0f} KiB")
            assert size < 1000 * 1000, size
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
