"""Step kinds of the nucleotide list form (phyml_amd/csrc/phyhip_kernels.hpp: kRecKindShift; chosen by fill_compact_records,
phyhip_queue.hip, from what the host knows about the tip rows; run by the straight-line bodies of nt2_run, phyhip_nt2.hpp;
profiles/r14_nt_step_kinds.md).  A step whose two children reach it in one of six ways over tip rows that are one-hot throughout
skips the tests that cannot fire there.  What can go wrong: a body's arithmetic or operand order, a matrix or tip dword taken from
the other child's slot, a kind handed out over a row that is not one-hot (or kept after the row was rewritten), and the all-ones
rule where a body takes it for impossible -- each shows in some internal partial vector or scale vector.

Check, through the C ABI: after Lk(NULL) EVERY internal partial vector and scale vector is np.array_equal to the oracle's
(tests/orc.py), lnL agrees with it and equals the all-stored twin's (set_virtual_buffers(0)) -- at the shapes of
tests/test_gpu_nt_records.py, at 300 taxa x (32 x CUs + 38) patterns (every kind in the four-lane bodies) and on a caterpillar
and a balanced tree, one- and both-sided, in three store settings, with

  onehot     every tip row one-hot
  one_row    one row (a cherry's aunt; balanced tree: the tip at the root) with N and R codes: the steps that read it must fall to kind 0
  all_n      columns that are N in a cherry and its aunt (balanced tree: in two more cherries whose sisters are cherries): the
             all-ones rule fires in lists whose other steps are specialised, also behind the vote of an in-step x forwarded step
  unscaled   apply_scaling off

and with a row rewritten from one-hot to ambiguous and back between traversals (the kinds must follow).  Every case asserts from
phyhip_get_step_kind_stats that each kind it is meant to drive occurs, in both step parities (driven_kinds below)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from gpu_common import synthetic_oracle
from phyml_amd import lktree, synth
from test_gpu_nt_chain import sisters_with_tip_aunt, written
from test_gpu_nt_records import mixed_patterns

SETTINGS = ["default", "all_stored", "unchained"]
VARIANTS = ["onehot", "one_row", "all_n", "unscaled"]
SHAPES = [("random", 300, 96, 7), ("random", 301, 96, 7), ("random", 40, "mixed", 3), ("random", 300, "mixed", 7), ("caterpillar", 33, 96, 11),
          ("balanced", 33, 96, 13)]


def caterpillar(n, seed):
    edges = [(n, 0), (n, 1)]
    for j in range(1, n - 2):
        edges += [(n + j, n + j - 1), (n + j, j + 1)]
    edges.append((2 * n - 3, n - 1))
    return edge_tree(n, edges, seed)


def balanced(n, seed):
    """two halves split in two down to cherries, and one tip, at the root: sisters that are both cherries occur"""
    edges, nxt = [], [n]

    def sub(tips):
        if len(tips) == 1:
            return tips[0]
        m = nxt[0]; nxt[0] += 1
        h = len(tips) // 2
        edges.append((m, sub(tips[:h]))); edges.append((m, sub(tips[h:])))
        return m

    r = nxt[0]; nxt[0] += 1
    h = (n - 1) // 2
    for part in (list(range(h)), list(range(h, n - 1)), [n - 1]):
        edges.append((r, sub(part)))
    return edge_tree(n, edges, seed)


def edge_tree(n, edges, seed):
    ne = 2 * n - 3
    assert len(edges) == ne
    u = synth.hash_u64(seed, 2, np.arange(ne)) >> np.uint64(11)
    lens = 0.02 + 0.28 * (u.astype(np.float64) / float(1 << 53))
    el = np.array([a for a, _ in edges], dtype=np.int32); er = np.array([b for _, b in edges], dtype=np.int32)
    return synth.EdgeTree(n, el, er, lens, ["T%05d" % i for i in range(n)])


def patterns(P):
    return mixed_patterns() if P == "mixed" else P


@functools.lru_cache(maxsize=None)
def alignment(topo, n_otu, P, seed):
    """(model, tree, characters, weights, (cherry tip, cherry tip, aunt tip)): read-only"""
    P = patterns(P)
    plain, tree, st, _, wg = synthetic_oracle(n_otu, P, 4, 4, seed)
    if topo != "random":
        tree = caterpillar(n_otu, seed) if topo == "caterpillar" else balanced(n_otu, seed)
        st = synth.simulate_states(tree, P, 4, seed)
    chars = synth.states_to_chars(st, 4)
    # (the balanced tree has no cherry with a tip aunt: its first cherry and the lone tip at the root)
    trio = (0, 1, n_otu - 1) if topo == "balanced" else sisters_with_tip_aunt(oracle_of(plain.m, tree, chars, wg, 1)[0])
    return plain.m, tree, chars, wg, trio


def oracle_of(m, tree, chars, wg, apply_scaling):
    tv, ds, amb = [], [], []
    for t in range(tree.n_otu):
        v, s, x = orc.init_tip(m.datatype, chars[t])
        tv.append(v); ds.append(s); amb.append(x)
    return orc.OracleTree(m, tree.n_otu, tree.edge_left, tree.edge_rght, tree.edge_len, wg, tv, ds, amb, apply_scaling=apply_scaling, arith=1), tv


def variant_chars(topo, chars, trio, variant):
    a, b, c = trio
    chars = chars.copy()
    if variant == "one_row":
        chars[c, 0::10] = ord("N"); chars[c, 5::10] = ord("R")
    elif variant == "all_n":
        rows = [a, b, c] + ([0, 1, 6, 7] if topo == "balanced" else [])
        for r in rows:
            chars[r, 0::5] = ord("N")
    return chars


@functools.lru_cache(maxsize=None)
def reference(topo, n_otu, P, seed, variant, both):
    """(oracle tree after Lk(NULL), its lnL, tree, tip vectors, weights): once per case, read-only"""
    m, tree, chars, wg, trio = alignment(topo, n_otu, P, seed)
    ot, tv = oracle_of(m, tree, variant_chars(topo, chars, trio, variant), wg, 0 if variant == "unscaled" else 1)
    return ot, ot.lk(None, both_sides=both), tree, tv, wg


def device_tree(ot, tree, tv, wg, apply_scaling=1):
    m = ot.m
    t = lktree.LkTree(ot.n, tree.edge_left, tree.edge_rght, tree.edge_len, len(wg), 4, 4, host_pmat=True)
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, apply_scaling)
    t.Make_Tree_For_Lk(wg)
    t.set_tips(tip_partials=tv)
    return t


def configure(t, setting, both):
    if setting == "all_stored":
        t.inst.set_virtual_buffers(0)
    elif setting == "unchained":
        t.inst.set_chained_buffers(0)
    t.Set_Both_Sides(both)


def kinds_of(t):
    return np.array(t.inst.step_kind_stats(), dtype=np.int64)   # [parity][kind]


def driven_kinds(topo, n_otu, P, setting, both):
    """The kinds a case is meant to drive, each in BOTH step parities -- or None where the launch's kernel carries no bodies and
    every step must be kind 0.  The kinds of a list follow from the tree, the traversal and the store setting alone (the host
    builds the list; no kernel is involved), so each set is a property of the shape:

      * which kernel: 96 patterns are one wave shape -- traverse_nt2_kernel<4, 2, ., 0, 2, INL>, which carries the bodies only
        with in-step children (nt2_bodied, phyhip_kernels.hpp), so a list in which every operation stores is kind 0 throughout;
        32 x CUs + 38 patterns run traverse_nt2_mixed_kernel, two- and four-lane bodies, in every setting;
      * without in-step children (every operation stores) only tip x forwarded steps can be specialised: kinds 1 and 2;
      * the 300- and 301-taxon random trees hold every one of the six kinds in both parities -- the shape that runs every
        four-lane body is 300 x (32 x CUs + 38);
      * a caterpillar is a chain of tip x forwarded steps: kind 1; its one cherry gives a single in-step step;
      * the balanced tree is cherries whose sisters are cherries: one is computed in the step, the other forwarded -- kind 3
        one-sided; in the pre-order half of a both-sided traversal the forwarded side may come first (kind 3 or 4);
      * the 40-taxon tree (seed 3) has forwarded x tip steps and the three in-step kinds 4, 5, 6 in both parities, kind 1 and
        kind 3 in one parity only; all stored, both orders of tip x forwarded in both."""
    mixed = P == "mixed"
    if setting == "all_stored":
        return (1, 2) if mixed and topo == "random" else None if not mixed else ()
    if topo == "caterpillar":
        return (1,)
    if topo == "balanced":
        return (3,) if not both else ((3, 4),)
    return (1, 2, 3, 4, 5, 6) if n_otu >= 300 else (2, 4, 5, 6)


def assert_buffers(t, ot, both):
    keys = list(ot.plk) if both else written(ot)
    assert len(keys) >= ot.n - 2
    for k in keys:
        assert np.array_equal(t.partials(*k), ot.plk[k]), k
        assert np.array_equal(t.scale_factors(*k), ot.scale[k]), k


@pytest.mark.parametrize("both", [False, True], ids=["one_sided", "both_sided"])
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("topo,n_otu,P,seed", SHAPES)
def test_every_internal_buffer_is_the_oracles(topo, n_otu, P, seed, variant, setting, both):
    ot, ref, tree, tv, wg = reference(topo, n_otu, P, seed, variant, both)
    scaling = 0 if variant == "unscaled" else 1
    t, t0 = device_tree(ot, tree, tv, wg, scaling), device_tree(ot, tree, tv, wg, scaling)
    try:
        configure(t, setting, both)
        t0.inst.set_virtual_buffers(0); t0.Set_Both_Sides(both)
        lnl, lnl0 = t.Lk(None), t0.Lk(None)
        kinds = kinds_of(t)
        print(f"{topo} {n_otu} x {len(wg)} {variant} {setting} both={both}: lnL {lnl!r} all-stored {lnl0!r} oracle {ref!r} kinds even {kinds[0]} odd {kinds[1]}")
        assert lnl == lnl0
        assert abs(lnl - ref) / abs(ref) < 1e-12
        want = driven_kinds(topo, n_otu, P, setting, both)
        if want is None:
            assert kinds[:, 1:].sum() == 0, kinds   # a kernel without bodies: the host hands out kind 0 throughout
        else:
            for parity in (0, 1):
                for kd in want:
                    got = sum(kinds[parity][k] for k in kd) if isinstance(kd, tuple) else kinds[parity][kd]
                    assert got > 0, (parity, kd, kinds)
                if n_otu >= 300:
                    assert kinds[parity][0] > 0      # ... next to generic steps (tip x tip, loaded children)
        if variant == "one_row":
            o1, r1, _, tv1, _ = reference(topo, n_otu, P, seed, "onehot", both)
            t1 = device_tree(o1, tree, tv1, wg)
            try:
                configure(t1, setting, both)
                t1.Lk(None)
                k1 = kinds_of(t1)
            finally:
                t1.close()
            assert kinds.sum() == k1.sum()
            if want is not None and not (topo == "balanced" and setting == "all_stored"):
                assert kinds[:, 1:].sum() < k1[:, 1:].sum(), (kinds, k1)   # the row's readers fell to kind 0
        if variant == "all_n" and both:   # (both directions: the cherry's buffer and the one above it and its aunt are written)
            ones = sum(int(np.any(np.all(np.asarray(ot.plk[k]).reshape(len(wg), -1) == 1.0, axis=1))) for k in written(ot))
            assert ones >= 2, ones
        assert_buffers(t, ot, both)
        assert t.Lk(None) == lnl
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("both", [False, True], ids=["one_sided", "both_sided"])
@pytest.mark.parametrize("topo,n_otu,P,seed", SHAPES)
def test_the_kinds_follow_a_rewritten_row(topo, n_otu, P, seed, both):
    """one-hot -> ambiguous -> one-hot, whole row and one pattern: the list is the same each time (a slot would serve it), its kinds are not"""
    o_hot, ref_hot, tree, tv_hot, wg = reference(topo, n_otu, P, seed, "onehot", both)
    o_amb, ref_amb, _, tv_amb, _ = reference(topo, n_otu, P, seed, "one_row", both)
    c = alignment(topo, n_otu, P, seed)[4][2]
    t = device_tree(o_hot, tree, tv_hot, wg)
    try:
        t.Set_Both_Sides(both)

        def run():
            before = kinds_of(t)
            lnl = t.Lk(None)
            return lnl, kinds_of(t) - before

        lnl, k_hot = run()
        assert abs(lnl - ref_hot) / abs(ref_hot) < 1e-12
        t.inst.set_tip_partials(c, tv_amb[c])
        lnl_a, k_amb = run()
        assert abs(lnl_a - ref_amb) / abs(ref_amb) < 1e-12
        assert k_amb.sum() == k_hot.sum() and k_amb[:, 1:].sum() < k_hot[:, 1:].sum(), (k_hot, k_amb)
        assert_buffers(t, o_amb, both)
        t.inst.set_tip_partials(c, tv_hot[c])
        lnl_b, k_back = run()
        assert lnl_b == lnl and np.array_equal(k_back, k_hot)
        assert_buffers(t, o_hot, both)
        # one pattern hidden (every state allowed) and restored, as the leave-one-out loop does
        t.inst.set_tip_partials_at_pattern(c, 5, np.ones(4))
        _, k_one = run()
        assert k_one[:, 1:].sum() < k_hot[:, 1:].sum(), (k_hot, k_one)
        t.inst.set_tip_partials_at_pattern(c, 5, np.asarray(tv_hot[c]).reshape(-1, 4)[5])
        lnl_c, k_rest = run()
        assert lnl_c == lnl and np.array_equal(k_rest, k_hot)
        print(f"{topo} {n_otu} both={both}: specialised steps {k_hot[:, 1:].sum()} -> {k_amb[:, 1:].sum()} -> {k_back[:, 1:].sum()} -> {k_one[:, 1:].sum()} -> {k_rest[:, 1:].sum()}")
    finally:
        t.close()
