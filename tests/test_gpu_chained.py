"""Chained buffers (include/phyhip.h: phyhip_set_chained_buffers, phyhip_get_chained_stats): a one-sided whole-tree traversal does
not store a forwarded result even when one of its children is itself unstored -- virtual, deferred, or chained earlier in the
list -- and whatever LEAVES through the interface is still the double the reference holds in t_edge::p_lk_* at that point: read
in list order or dependant first, and after a tip row, a matrix or a buffer under the chain has changed.

Oracle: tests/orc.py (the pinned CPU restatement) and the same device tree with every buffer stored (set_virtual_buffers(0)).
`Replay` restates the host's rules (rewrite_pending, the two passes of defer_forwarded) on the oracle tree's own post-order, so that
the tests know WHICH buffers are chained and can aim at them; the device's counters are held to its counts.  The chain threshold is
lowered to 3 operations through its own setter, the virtual threshold through phyhip_set_virtual_buffers, as test_gpu_deferred.py
does; the shapes are that file's."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_common import synthetic_pair

# (states, categories, patterns, taxa, seed, shards): 9 taxa / seed 2 launch a rewritten list of 5 operations (odd: padded with a
# re-run of the last one), 12 taxa / seed 1 one of 8.  200 patterns: one wave shape, a partly filled wave; 9 000: the two-shape
# launch; 20 states at small_aa_16x600's size; two pattern shards on one device.
SHAPES = [(4, 4, 200, 9, 2, None), (4, 4, 200, 12, 1, None), (4, 4, 9000, 9, 2, None), (4, 4, 9000, 12, 1, None),
          (20, 4, 600, 16, 6, None), (4, 4, 700, 12, 1, (0, 0))]
IDS = ["nt_200_odd", "nt_200_even", "nt_9000_odd", "nt_9000_even", "aa_16x600", "nt_two_shards"]
LIST_LENGTH = {(9, 2): 5, (12, 1): 8}


class Replay:
    """The rewritten list of a one-sided Lk(NULL) as phyhip_unstored.hip builds it, on node numbers.  m: its length; virt: nodes left
    virtual; deferred / chained: {node: [child nodes]}; key: node -> (edge, side); order: the nodes in post-order."""

    def __init__(self, ot, min_ops=3):
        n, r = ot.n, ot.tip_root
        v0 = ot.adj[r][0][0]
        order = []
        ot.post_order(r, v0, order)
        ops, self.key = [], {}
        for (e, d) in order:
            ops.append((d, [v for (v, be) in ot.adj[d] if be != e]))
            self.key[d] = (e, 0 if d == ot.el[e] else 1)
        self.order = [d for (_, d) in order]
        assert len(ops) >= max(min_ops, 3) and sum(1 for _, k in ops if max(k) >= n) >= 3
        ee, virt, L = (r, v0), set(), []
        for d, (c1, c2) in ops:
            if c1 < n and c2 < n and d not in ee:
                virt.add(d)
                continue
            inl, used = [False, False], False
            for w, c in enumerate((c1, c2)):
                if c in virt:
                    if not used and c1 != c2:
                        inl[w] = used = True
                    else:
                        L.append(dict(dest=c, c=(0, 0), nostore=True, inl=(False, False)))
            L.append(dict(dest=d, c=(c1, c2), nostore=False, inl=tuple(inl)))
        m = len(L)
        if m & 1 and L[m - 3]["nostore"] and L[m - 3]["dest"] in L[-1]["c"]:
            L[m - 3]["nostore"] = False
            virt.discard(L[m - 3]["dest"])
        last_w, last_r = {}, {}
        for k, o in enumerate(L):
            assert o["dest"] not in last_w  # (a post-order writes every buffer once)
            last_w[o["dest"]] = k
            for w, c in enumerate(o["c"]):
                if c >= n and not o["inl"][w]:
                    last_r[c] = k

        def forwarded(i, o):
            if o["nostore"] or o["dest"] in ee or not (i < last_r.get(o["dest"], -1) <= i + 2):
                return False
            return not (m & 1 and i + 3 == m and o["dest"] in L[-1]["c"])
        deferred, chained = {}, {}
        for i, o in enumerate(L[:-1]):   # defer_forwarded's first pass: every child a tip or in memory after the launch
            if forwarded(i, o) and not any(c >= n and (o["inl"][w] or c in virt or c in deferred or last_w.get(c, -1) >= i)
                                           for w, c in enumerate(o["c"])):
                deferred[o["dest"]] = list(o["c"])
        if m >= min_ops:                 # its second pass, on a list that chains: every child a tip or not written again behind the operation
            for i, o in enumerate(L[:-1]):   # (a post-order: every edge has its own matrix)
                if o["dest"] not in deferred and forwarded(i, o) and not any(c >= n and last_w.get(c, -1) >= i for c in o["c"]):
                    chained[o["dest"]] = list(o["c"])
        self.m, self.virt, self.deferred, self.chained, self.n = m, virt, deferred, chained, n

    def unstored(self, d):
        return d in self.virt or d in self.deferred or d in self.chained

    def depth(self, d):
        """definitions on the longest path below d that are unstored, d's own included"""
        kids = self.chained.get(d) or self.deferred.get(d) or []
        return 1 + max([self.depth(c) for c in kids if c >= self.n and self.unstored(c)] + [0])

    def tip_under(self, d):
        """a tip read by a deferred or chained definition among the unstored inputs of d, transitively"""
        stack = [d]
        while stack:
            x = stack.pop()
            kids = self.chained.get(x) or self.deferred.get(x) or []
            if x != d and min(kids + [self.n]) < self.n:
                return min(kids)
            stack += [k for k in kids if k >= self.n and self.unstored(k)]
        return None

    def mid_chain(self):
        """(dependant, input): both chained or deferred, the input unstored itself -- a buffer in the middle of a chain"""
        for d in self.order:
            for c in self.chained.get(d, []):
                if c in self.chained or c in self.deferred:
                    return d, c
        return None


def pair(shape, host_pmat=True):
    ns, C, P, n_otu, seed, devices = shape
    dev = None if devices is None else list(devices)
    t, ot, _, _ = synthetic_pair(n_otu, P, ns, C, seed=seed, host_pmat=host_pmat, ambiguous_every=13, devices=dev)
    t0, _, _, _ = synthetic_pair(n_otu, P, ns, C, seed=seed, host_pmat=host_pmat, ambiguous_every=13, devices=dev)
    t.inst.set_virtual_buffers(3)
    t.inst.set_chained_buffers(3)
    t0.inst.set_virtual_buffers(0)
    ot.lk(None)  # (the oracle's vectors of the one-sided traversal: what one_sided_keys reads)
    return t, t0, ot


def one_sided_keys(ot, rp):
    """the buffers a one-sided traversal writes, in list order"""
    keys = [rp.key[d] for d in rp.order]
    assert sorted(keys) == sorted(k for k in ot.plk if np.any(ot.plk[k] != 0))
    return keys


def copies(t0, keys):
    return {k: (t0.partials(*k).copy(), t0.scale_factors(*k).copy()) for k in keys}


def assert_reads_back(t, k, want):
    assert np.array_equal(t.partials(*k), want[0]), k
    assert np.array_equal(t.scale_factors(*k), want[1]), k


def edge_between(ot, a, b):
    return [be for (v, be) in ot.adj[a] if v == b][0]


def test_the_chosen_trees_give_chains():
    from gpu_common import synthetic_oracle
    for (n_otu, seed), want in list(LIST_LENGTH.items()) + [((16, 6), None)]:
        rp = Replay(synthetic_oracle(n_otu, 8, 4, 4, seed)[0])
        assert want is None or rp.m == want
        assert len(rp.chained) >= 2 and max(rp.depth(d) for d in rp.chained) >= 3 and rp.mid_chain(), (n_otu, seed, rp.m, rp.chained)
        assert rp.tip_under(rp.mid_chain()[0]) is not None
    assert {m & 1 for m in LIST_LENGTH.values()} == {0, 1}


@pytest.mark.parametrize("reverse", [False, True], ids=["list_order", "dependant_first"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_sided_traversal_chains_and_reads_back_bit_equal(shape, reverse):
    t, t0, ot = pair(shape)
    try:
        lnl, lnl0 = t.Lk(None), t0.Lk(None)
        ref = ot.lk(None)
        assert lnl == lnl0                       # the same double whether the stores were left out or not
        assert abs(lnl - ref) / abs(ref) < 1e-12
        rp = Replay(ot)
        now = len(rp.chained)
        assert now >= 2 and t.inst.chained_stats() == (now, now, 0, 0)
        nd = len(rp.deferred)
        assert t.inst.deferred_stats() == (nd, nd, 0, 0)                         # (what they meant before)
        vnow, vskipped, _, vstored = t.inst.virtual_stats()
        assert (vnow, vskipped, vstored) == (len(rp.virt), len(rp.virt), 0)
        assert t0.inst.chained_stats() == (0, 0, 0, 0)
        # a second traversal: every old definition is dropped, nothing is stored for it, the same buffers are chained again
        assert t.Lk(None) == lnl0
        assert t.inst.chained_stats() == (now, 2 * now, 0, now)
        assert t.inst.deferred_stats() == (nd, 2 * nd, 0, nd) and t.inst.virtual_stats()[3] == 0
        # reading back stores: every buffer bit-equal to the oracle and to the storing run -- inputs first, or dependants first
        keys = one_sided_keys(ot, rp)
        for k in (keys[::-1] if reverse else keys):
            got, sc = t.partials(*k), t.scale_factors(*k)
            assert np.array_equal(got, ot.plk[k]), k
            assert np.array_equal(sc, ot.scale[k]), k
            assert np.array_equal(got, t0.partials(*k)), k
            assert np.array_equal(sc, t0.scale_factors(*k)), k
        assert t.inst.chained_stats() == (0, 2 * now, now, now)
        assert t.inst.deferred_stats() == (0, 2 * nd, nd, nd)
        assert t.inst.virtual_stats()[0] == 0 and t.inst.virtual_stats()[3] == len(rp.virt)
        # the chained class has its own switch; phyhip_set_virtual_buffers(0) stores all three classes and stops all three
        assert t.Lk(None) == lnl0 and t.inst.chained_stats()[0] == now
        t.inst.set_chained_buffers(0)
        assert t.Lk(None) == lnl0 and t.inst.chained_stats()[0] == 0 and t.inst.deferred_stats()[0] == nd
        t.inst.set_chained_buffers(3)
        assert t.Lk(None) == lnl0 and t.inst.chained_stats()[0] == now
        t.inst.set_virtual_buffers(0)
        assert t.inst.chained_stats()[0] == 0 and t.inst.deferred_stats()[0] == 0 and t.inst.virtual_stats()[0] == 0
        assert t.Lk(None) == lnl0 and t.inst.chained_stats()[0] == 0
        for k in keys:
            assert_reads_back(t, k, (ot.plk[k], ot.scale[k]))
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("host_pmat", [True, False], ids=["uploaded_matrices", "device_built_matrices"])
def test_a_chain_keeps_its_values_when_matrices_or_tips_change(shape, host_pmat):
    """A tip row under a chain, one matrix under a chain (the upload route moves the old value to a snapshot slot, the device route
    stores the dependant and its inputs first), every matrix of the tree one call at a time."""
    t, t0, ot = pair(shape, host_pmat=host_pmat)
    try:
        rp = Replay(ot)
        keys = one_sided_keys(ot, rp)
        d, c = rp.mid_chain()
        # (1) a tip row under a chain: below the input of a chained definition
        tip = rp.tip_under(d)
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        for x in (t, t0):
            x.inst.set_tip_partials_at_pattern(tip, 3, np.ones(shape[0]))
        for k in keys[::-1]:
            assert_reads_back(t, k, before[k])
        # (2) one matrix under a chain: the one the dependant reads its chained input through
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        now, _, on_demand, _ = t.inst.chained_stats()
        assert now == len(rp.chained)
        for x in (t, t0):
            x.edge(edge_between(ot, d, c)).contents.l = 0.37
            x.Update_PMat_At_Given_Edge(edge_between(ot, d, c))
        if host_pmat:
            assert t.inst.chained_stats()[2] == on_demand          # (a snapshot: nothing stored)
        else:
            assert t.inst.chained_stats()[2] > on_demand           # (stored first, with its inputs)
        for k in keys:
            assert_reads_back(t, k, before[k])
        # (3) every matrix changes without a traversal, one call per edge
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        on_demand = t.inst.chained_stats()[2]
        lens = np.linspace(0.01, 0.5, t.ne)
        if host_pmat:
            for e in range(t.ne):
                for x in (t, t0):
                    x.edge(e).contents.l = float(lens[e])
                    x.Update_PMat_At_Given_Edge(e)
            assert t.inst.chained_stats()[0] == len(rp.chained) and t.inst.chained_stats()[2] == on_demand   # snapshots
        else:  # (fewer than 32 matrices in one call: dependants are stored first; the batch route has a test of its own below)
            idx = np.array([t.edge(e).contents.Pij_rr_idx for e in range(t.ne)], dtype=np.int32)
            for x in (t, t0):
                x.inst.update_transition_matrices(idx, lens)
                for e in range(t.ne):
                    x.edge(e).contents.l = float(lens[e])
        for k in keys[::-1]:
            assert_reads_back(t, k, before[k])
        assert t.Lk(None) == t0.Lk(None)
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", [(4, 4, 200, 34, 21, None), (20, 4, 90, 34, 21, None)], ids=["nt", "aa"])
def test_a_whole_tree_batch_of_device_built_matrices_moves_definitions_to_snapshot_slots(shape):
    """Update_All_PMat as one call of at least 32 matrices, behind a one-sided traversal at the library's own thresholds: pmat_kernel
    moves every old value a definition reads into the buffer's snapshot slots; nothing is stored until somebody reads."""
    ns, C, P, n_otu, seed, _ = shape
    t, ot, _, _ = synthetic_pair(n_otu, P, ns, C, seed=seed, host_pmat=False, ambiguous_every=13)
    t0, _, _, _ = synthetic_pair(n_otu, P, ns, C, seed=seed, host_pmat=False, ambiguous_every=13)
    try:
        t0.inst.set_virtual_buffers(0)
        ot.lk(None)
        rp = Replay(ot, min_ops=16)
        keys = one_sided_keys(ot, rp)
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        idx = np.array([t.edge(e).contents.Pij_rr_idx for e in range(t.ne)], dtype=np.int32)
        lens = np.linspace(0.01, 0.5, t.ne)
        assert len(idx) >= 32
        for x in (t, t0):
            x.inst.update_transition_matrices(idx, lens)
            for e in range(t.ne):
                x.edge(e).contents.l = float(lens[e])
        now, _, on_demand, _ = t.inst.chained_stats()
        assert now == len(rp.chained) >= 10 and on_demand == 0
        assert t.inst.deferred_stats()[0] == len(rp.deferred) and t.inst.deferred_stats()[2] == 0
        for k in keys[::-1]:
            assert_reads_back(t, k, before[k])
        assert t.inst.chained_stats()[2] == len(rp.chained)
        assert t.Lk(None) == t0.Lk(None)
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_chain_keeps_its_values_when_a_buffer_in_its_middle_is_rewritten(shape):
    """Update_Partial_Lk rewrites a buffer in the middle of a chain (below it a matrix has changed, so the new content differs),
    then Lk(b) at that edge; phyhip_set_partials overwrites such a buffer: dependants keep the old content."""
    t, t0, ot = pair(shape)
    try:
        rp = Replay(ot)
        keys = one_sided_keys(ot, rp)
        d, c = rp.mid_chain()
        e_c = edge_between(ot, d, c)
        k_c = rp.key[c]
        assert k_c[0] == e_c
        below = [be for (v, be) in ot.adj[c] if v != d][0]
        # every buffer written once (both sides), then the one-sided traversal that chains
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)
        assert t.inst.chained_stats()[0] == 0          # (a both-sided list shares its matrices: never chained)
        for x in (t, t0):
            x.Set_Both_Sides(False)
        assert t.Lk(None) == t0.Lk(None)
        assert t.inst.chained_stats()[0] == len(rp.chained)
        before = copies(t0, keys)
        on_demand = t.inst.chained_stats()[2]
        for x in (t, t0):
            x.edge(below).contents.l = 0.41
            x.Update_PMat_At_Given_Edge(below)
            x.Update_Partial_Lk(e_c, c)
        assert t.Lk(e_c) == t0.Lk(e_c)
        assert t.inst.chained_stats()[2] >= on_demand + 1      # the launch that writes the input stored its dependant first
        assert np.array_equal(t.partials(*k_c), t0.partials(*k_c))
        assert not np.array_equal(t0.partials(*k_c), before[k_c][0])
        for k in keys[::-1]:
            if k != k_c:
                assert_reads_back(t, k, before[k])
        assert t.inst.chained_stats()[0] == 0
        # phyhip_set_partials on the same input, chained again
        assert t.Lk(None) == t0.Lk(None)
        assert t.inst.chained_stats()[0] == len(rp.chained)
        before = copies(t0, keys)
        new = before[k_c][0] * 0.5
        for x in (t, t0):
            x.inst.set_partials(x.side_buffer(*k_c), new)
        assert np.array_equal(t.partials(*k_c), t0.partials(*k_c))
        assert not np.array_equal(t0.partials(*k_c), before[k_c][0])
        for k in keys[::-1]:
            if k != k_c:
                assert_reads_back(t, k, before[k])
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("reader", ["update_eigen_lr", "exact_site_lk"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_readers_outside_the_traversal_launch_store_a_mid_chain_buffer_in_order(shape, reader):
    """Readers that store what they read and launch on their own, at the edge below a buffer in the middle of a chain, behind a
    one-sided traversal: `Update_Eigen_Lr` (it rewrites its queue once WITHOUT launching, and the launch rewrites it again: the
    definitions already standing in front must keep their places, and the dependant stays unstored behind them) and the exact
    per-site route.  The reader's own values, then the dependant first, then every buffer."""
    t, t0, ot = pair(shape)
    try:
        rp = Replay(ot)
        keys = one_sided_keys(ot, rp)
        d, c = rp.mid_chain()
        e_c = edge_between(ot, d, c)
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)          # (every buffer written once: both sides of e_c hold values)
        for e in range(t.ne):                     # ... and what memory holds of a chained buffer is NOT what the next traversal defines
            for x in (t, t0):
                x.edge(e).contents.l = 0.02 + 0.01 * (e % 17)
                x.Update_PMat_At_Given_Edge(e)
        for x in (t, t0):
            x.Set_Both_Sides(False)
        assert t.Lk(None) == t0.Lk(None)
        now, _, on_demand, _ = t.inst.chained_stats()
        assert now == len(rp.chained)
        before = copies(t0, keys)
        got, ref = [], []
        for x, out in ((t, got), (t0, ref)):
            if reader == "update_eigen_lr":
                x.Set_Update_Eigen_Lr(True); x.Update_Eigen_Lr(e_c); x.Set_Update_Eigen_Lr(False)
                x.Set_Use_Eigen_Lr(True)
                out.append(x.dLk(0.07, e_c)[1]); out.append(x.c_dlnL)
                x.Set_Use_Eigen_Lr(False)
            else:
                out.extend(x.Exact_Site_Lk(e_c))
        # (9 000 patterns: a launch with stored definitions in front is of the list form and adds its block sums in two wave shapes, the
        # all-stored run's in one -- the same patterns, other partial sums; the exact route is the same double everywhere)
        if reader == "update_eigen_lr" and shape[2] >= 8192:
            assert all(abs(u - v) <= 1e-9 * max(1.0, abs(v)) for u, v in zip(got, ref)), (got, ref)
        else:
            assert all(np.array_equal(u, v) for u, v in zip(got, ref)), (got, ref)
        assert t.inst.chained_stats()[2] > on_demand         # the input was stored, with its own inputs
        assert_reads_back(t, rp.key[d], before[rp.key[d]])   # the dependant: behind its input, on the input's stored value
        for k in keys[::-1]:
            assert_reads_back(t, k, before[k])
        assert t.Lk(None) == t0.Lk(None)
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_both_sides_never_chain(shape):
    t, t0, ot = pair(shape)
    try:
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)
        assert t.inst.chained_stats() == (0, 0, 0, 0)
        for b in range(t.ne):
            assert t.Lk(b) == t0.Lk(b), b
        assert t.Lk(None) == t0.Lk(None)
        assert t.inst.chained_stats() == (0, 0, 0, 0)
        for k in ot.plk:
            assert_reads_back(t, k, (t0.partials(*k), t0.scale_factors(*k)))
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("ns,C,P,devices", [(4, 4, 300, None), (20, 4, 90, None), (4, 4, 700, (0, 0))])
@pytest.mark.parametrize("host_pmat", [True, False])
def test_random_call_streams_keep_the_stored_runs_scalars(ns, C, P, devices, host_pmat):
    """The stream of test_gpu_virtual.py with full traversals that are one-sided half of the time (the ones that chain), subtree
    post-orders (one-sided lists of their own), and both thresholds moving: every scalar equal to the run that stores every buffer,
    and every buffer read back at the end."""
    dev = None if devices is None else list(devices)
    t, ot, tree, st = synthetic_pair(34, P, ns, C, seed=21, host_pmat=host_pmat, ambiguous_every=13, devices=dev)
    t0, _, _, _ = synthetic_pair(34, P, ns, C, seed=21, host_pmat=host_pmat, ambiguous_every=13, devices=dev)
    try:
        t0.inst.set_virtual_buffers(0)
        t.inst.set_chained_buffers(3)
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)   # (every buffer written once)
        rng = np.random.default_rng(int(os.environ.get("PHYHIP_FUZZ_SEED", "23")))
        internal = [e for e in range(t.ne) if ot.el[e] >= ot.n and ot.er[e] >= ot.n]
        keys = list(ot.plk)
        chained_seen = 0
        for it in range(int(os.environ.get("PHYHIP_FUZZ_ITERS", "300"))):
            act = int(rng.integers(0, 11))
            if act in (0, 10):
                both = bool(rng.integers(0, 2))
                for x in (t, t0):
                    x.Set_Both_Sides(both)
                assert t.Lk(None) == t0.Lk(None), it
                chained_seen += t.inst.chained_stats()[0]
            elif act in (1, 2):
                for e in rng.choice(t.ne, size=int(rng.integers(1, 6)), replace=False):
                    l = float(rng.uniform(0.005, 0.4))
                    for x in (t, t0):
                        x.edge(int(e)).contents.l = l
                        x.Update_PMat_At_Given_Edge(int(e))
            elif act == 3:
                e = int(rng.choice(internal))
                a, d = (int(ot.el[e]), int(ot.er[e])) if rng.integers(0, 2) else (int(ot.er[e]), int(ot.el[e]))
                for x in (t, t0):
                    x.Post_Order_Lk(a, d)      # the whole subtree behind d: a long one-sided list
                if it % 2:
                    l = float(rng.uniform(0.005, 0.4))
                    for x in (t, t0):
                        x.edge(e).contents.l = l
                        x.Update_PMat_At_Given_Edge(e)
                assert t.Lk(e) == t0.Lk(e), it
            elif act == 4:
                e = int(rng.integers(0, t.ne))
                if it % 3 == 0 and ot.el[e] >= ot.n:
                    l = float(rng.uniform(0.005, 0.4))
                    for x in (t, t0):
                        x.Update_Partial_Lk(e, int(ot.el[e]))
                        x.edge(e).contents.l = l
                        x.Update_PMat_At_Given_Edge(e)
                assert t.Lk(e) == t0.Lk(e), it
            elif act == 5:
                e = int(rng.choice(internal))
                got, ref = [], []
                for x, out in ((t, got), (t0, ref)):
                    x.Set_Update_Eigen_Lr(True); x.Set_Use_Eigen_Lr(False)
                    out.append(x.Lk(e))
                    x.Set_Update_Eigen_Lr(False); x.Set_Use_Eigen_Lr(True)
                    out.append(x.dLk(0.11, e)[1]); out.append(x.c_dlnL)
                    x.Set_Use_Eigen_Lr(False)
                assert got == ref, it
            elif act in (6, 7):
                for _ in range(int(rng.integers(1, 4))):
                    e = int(rng.integers(0, t.ne))
                    d = int(ot.el[e] if rng.integers(0, 2) else ot.er[e])
                    if d >= ot.n:
                        for x in (t, t0):
                            x.Update_Partial_Lk(e, d)
            elif act == 8:
                k = keys[int(rng.integers(0, len(keys)))]     # a host reader at a random moment
                assert np.array_equal(t.partials(*k), t0.partials(*k)), (it, k)
                assert np.array_equal(t.scale_factors(*k), t0.scale_factors(*k)), (it, k)
            elif it % 4 == 0:
                t.inst.set_virtual_buffers(int(rng.choice([0, 2, 16, 40])))   # (the thresholds move; 0 stores what is unstored)
                t.inst.set_chained_buffers(int(rng.choice([0, 3, 3, 16])))
            else:
                tip, pat = int(rng.integers(0, ot.n)), int(rng.integers(0, P))
                v = np.zeros(ns); v[int(rng.integers(0, ns))] = 1.0
                if rng.integers(0, 2):
                    v[:] = 1.0
                for x in (t, t0):
                    x.inst.set_tip_partials_at_pattern(tip, pat, v)
        assert chained_seen > 0
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)
        for k in ot.plk:
            assert np.array_equal(t.partials(*k), t0.partials(*k)), k
            assert np.array_equal(t.scale_factors(*k), t0.scale_factors(*k)), k
    finally:
        t.close(); t0.close()
