"""Deferred buffers (include/phyhip.h: phyhip_set_virtual_buffers, phyhip_get_deferred_stats): a whole-tree traversal does not
store a result that every reader takes from registers when its children are tips or stored buffers -- and whatever LEAVES through
the interface is still the double the reference holds in t_edge::p_lk_* at that point, also after a buffer the definition reads,
one of its matrices or one of its tip rows has changed.

Oracle: tests/orc.py (the pinned CPU restatement) and the same device tree with every buffer stored (set_virtual_buffers(0)).
`replay` restates the host's rule on the oracle tree's own post-order, so that the tests know WHICH buffers are deferred and can
aim at them; the device's counter is held to its count."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_common import synthetic_pair

# (states, categories, patterns, taxa, seed, shards).  The threshold is lowered to 3 operations, so trees of 9 and 12 taxa qualify:
# 9 taxa / seed 2 launch a rewritten list of 5 operations (odd: padded with a re-run of the last one), 12 taxa / seed 1 one of 8.
# 200 patterns: one wave shape, a partly filled wave; 9 000: the two-shape launch; 20 states at small_aa_16x600's size; two pattern
# shards on one device.
SHAPES = [(4, 4, 200, 9, 2, None), (4, 4, 200, 12, 1, None), (4, 4, 9000, 9, 2, None), (4, 4, 9000, 12, 1, None),
          (20, 4, 600, 16, 6, None), (4, 4, 700, 12, 1, (0, 0))]
IDS = ["nt_200_odd", "nt_200_even", "nt_9000_odd", "nt_9000_even", "aa_16x600", "nt_two_shards"]
LIST_LENGTH = {(9, 2): 5, (12, 1): 8}


def replay(ot, min_ops=3):
    """The rewritten list of a one-sided Lk(NULL) as phyhip_unstored.hip builds it (rewrite_pending, then defer_forwarded), on node
    numbers: (list length, {deferred node: (edge, side, [child nodes])}, number of virtual buffers)."""
    n, r = ot.n, ot.tip_root
    v0 = ot.adj[r][0][0]
    order = []
    ot.post_order(r, v0, order)
    ops, key = [], {}
    for (e, d) in order:
        ops.append((d, [v for (v, be) in ot.adj[d] if be != e]))
        key[d] = (e, 0 if d == ot.el[e] else 1)
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
    deferred = {}
    for i, o in enumerate(L[:-1]):
        if o["nostore"] or o["dest"] in ee or not (i < last_r.get(o["dest"], -1) <= i + 2):
            continue
        if any(c >= n and (o["inl"][w] or c in virt or c in deferred or last_w.get(c, -1) >= i) for w, c in enumerate(o["c"])):
            continue
        if m & 1 and i + 3 == m and o["dest"] in L[-1]["c"]:
            continue
        deferred[o["dest"]] = key[o["dest"]] + (list(o["c"]),)
    return m, deferred, len(virt)


def pair(shape, host_pmat=True):
    ns, C, P, n_otu, seed, devices = shape
    dev = None if devices is None else list(devices)
    t, ot, _, _ = synthetic_pair(n_otu, P, ns, C, seed=seed, host_pmat=host_pmat, ambiguous_every=13, devices=dev)
    t0, _, _, _ = synthetic_pair(n_otu, P, ns, C, seed=seed, host_pmat=host_pmat, ambiguous_every=13, devices=dev)
    t.inst.set_virtual_buffers(3)
    t0.inst.set_virtual_buffers(0)
    ot.lk(None)  # (the oracle's vectors of the one-sided traversal: what one_sided_keys reads)
    return t, t0, ot


def one_sided_keys(ot):
    return [k for k in ot.plk if np.any(ot.plk[k] != 0)]


def copies(t0, keys):
    return {k: (t0.partials(*k).copy(), t0.scale_factors(*k).copy()) for k in keys}


def assert_reads_back(t, k, want):
    assert np.array_equal(t.partials(*k), want[0]), k
    assert np.array_equal(t.scale_factors(*k), want[1]), k


def edge_between(ot, a, b):
    return [be for (v, be) in ot.adj[a] if v == b][0]


def test_the_chosen_trees_give_an_odd_and_an_even_list():
    from gpu_common import synthetic_oracle
    for (n_otu, seed), want in LIST_LENGTH.items():
        m, deferred, _ = replay(synthetic_oracle(n_otu, 8, 4, 4, seed)[0])
        assert m == want and len(deferred) >= 2, (n_otu, seed, m, deferred)
    assert {m & 1 for m in LIST_LENGTH.values()} == {0, 1}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_sided_traversal_defers_and_reads_back_bit_equal(shape):
    t, t0, ot = pair(shape)
    try:
        lnl, lnl0 = t.Lk(None), t0.Lk(None)
        ref = ot.lk(None)
        assert lnl == lnl0                       # the same double whether the stores were deferred or not
        assert abs(lnl - ref) / abs(ref) < 1e-12
        _, want, n_virtual = replay(ot)
        now, total, on_demand, dropped = t.inst.deferred_stats()
        assert now > 0 and (now, total, on_demand, dropped) == (len(want), len(want), 0, 0)
        vnow, vskipped, _, vstored = t.inst.virtual_stats()                      # (what they meant before)
        assert (vnow, vskipped, vstored) == (n_virtual, n_virtual, 0)
        assert t0.inst.deferred_stats() == (0, 0, 0, 0)
        # a second traversal: every old definition is dropped, nothing is stored for it, the same buffers are deferred again
        assert t.Lk(None) == lnl0
        assert t.inst.deferred_stats() == (now, 2 * now, 0, now)
        assert t.inst.virtual_stats()[3] == 0
        # reading back stores: every buffer bit-equal to the oracle and to the storing run, nothing deferred afterwards
        for k in one_sided_keys(ot):
            got, sc = t.partials(*k), t.scale_factors(*k)
            assert np.array_equal(got, ot.plk[k]), k
            assert np.array_equal(sc, ot.scale[k]), k
            assert np.array_equal(got, t0.partials(*k)), k
            assert np.array_equal(sc, t0.scale_factors(*k)), k
        assert t.inst.deferred_stats() == (0, 2 * now, now, now)
        assert t.inst.virtual_stats()[0] == 0 and t.inst.virtual_stats()[3] == n_virtual
        # everything stored and no more deferring
        assert t.Lk(None) == lnl0 and t.inst.deferred_stats()[0] == now
        t.inst.set_virtual_buffers(0)
        assert t.inst.deferred_stats()[0] == 0 and t.inst.virtual_stats()[0] == 0
        assert t.Lk(None) == lnl0 and t.inst.deferred_stats()[0] == 0
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_deferred_buffer_keeps_its_value_when_an_input_is_rewritten(shape):
    """Update_Partial_Lk rewrites a buffer a deferred definition reads (below it a pendant matrix has changed, so the new content
    differs): the launch that writes it stores the dependant first, on the old content."""
    t, t0, ot = pair(shape)
    try:
        _, want, _ = replay(ot)
        hit = 0
        for d, (e, side, kids) in want.items():
            inner = [c for c in kids if c >= ot.n]
            if not inner:
                continue
            c = inner[0]
            e_c = edge_between(ot, d, c)
            below = [be for (v, be) in ot.adj[c] if v != d][0]
            assert t.Lk(None) == t0.Lk(None)
            keys = one_sided_keys(ot)
            before = copies(t0, keys)
            on_demand = t.inst.deferred_stats()[2]
            for x in (t, t0):
                x.edge(below).contents.l = 0.41
                x.Update_PMat_At_Given_Edge(below)
                x.Update_Partial_Lk(e_c, c)
            k_c = (e_c, 0 if c == ot.el[e_c] else 1)
            assert np.array_equal(t.partials(*k_c), t0.partials(*k_c))       # (the launch that writes the input)
            assert not np.array_equal(t0.partials(*k_c), before[k_c][0])
            assert t.inst.deferred_stats()[2] >= on_demand + 1              # ... stored its dependant (all of them, if it reads a virtual buffer)
            assert_reads_back(t, (e, side), before[(e, side)])
            for k in keys:
                if k != k_c:
                    assert_reads_back(t, k, before[k])
            assert t.inst.deferred_stats()[0] == 0
            hit += 1
            if hit == 2:
                break
        assert hit > 0
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("host_pmat", [True, False], ids=["uploaded_matrices", "device_built_matrices"])
def test_a_deferred_buffer_keeps_its_value_when_matrices_or_tips_change(shape, host_pmat):
    """A whole-tree matrix refresh (snapshot slots), one edge's matrix, and a tip row under a tip x inner definition."""
    t, t0, ot = pair(shape, host_pmat=host_pmat)
    try:
        _, want, _ = replay(ot)
        keys = one_sided_keys(ot)
        # (1) every matrix changes without a traversal
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        lens = np.linspace(0.01, 0.5, t.ne)
        if host_pmat:
            for e in range(t.ne):
                for x in (t, t0):
                    x.edge(e).contents.l = float(lens[e])
                    x.Update_PMat_At_Given_Edge(e)
            now, _, on_demand, _ = t.inst.deferred_stats()
            assert now == len(want) and on_demand == 0       # an upload moves the old value to a snapshot slot: nothing stored
        else:  # (fewer than 32 matrices in one call: dependants are stored first; the batch route has a test of its own below)
            idx = np.array([t.edge(e).contents.Pij_rr_idx for e in range(t.ne)], dtype=np.int32)
            for x in (t, t0):
                x.inst.update_transition_matrices(idx, lens)
                for e in range(t.ne):
                    x.edge(e).contents.l = float(lens[e])
        for k in keys:
            assert_reads_back(t, k, before[k])
        # (2) one edge's matrix, read by a deferred definition
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        d, (e, side, kids) = next(iter(want.items()))
        for x in (t, t0):
            x.edge(edge_between(ot, d, kids[0])).contents.l = 0.37
            x.Update_PMat_At_Given_Edge(edge_between(ot, d, kids[0]))
        for k in keys:
            assert_reads_back(t, k, before[k])
        # (3) a tip row under a tip x inner definition
        mixed = [(d, v) for d, v in want.items() if min(v[2]) < ot.n <= max(v[2])]
        assert mixed, want
        d, (e, side, kids) = mixed[0]
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        ns = shape[0]
        for x in (t, t0):
            x.inst.set_tip_partials_at_pattern(min(kids), 3, np.ones(ns))
        assert t.inst.deferred_stats()[0] == len(want) - 1   # (stored before the row changed: it alone)
        for k in keys:
            assert_reads_back(t, k, before[k])
        assert t.Lk(None) == t0.Lk(None)
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", [(4, 4, 200, 34, 21, None), (20, 4, 90, 34, 21, None)], ids=["nt", "aa"])
def test_a_whole_tree_batch_of_device_built_matrices_moves_definitions_to_snapshot_slots(shape):
    """Update_All_PMat as one call of at least 32 matrices: pmat_kernel moves every old value a definition reads into the buffer's
    snapshot slots; nothing is stored until somebody reads."""
    t, t0, ot = pair(shape, host_pmat=False)
    try:
        _, want, _ = replay(ot)
        keys = one_sided_keys(ot)
        assert t.Lk(None) == t0.Lk(None)
        before = copies(t0, keys)
        idx = np.array([t.edge(e).contents.Pij_rr_idx for e in range(t.ne)], dtype=np.int32)
        lens = np.linspace(0.01, 0.5, t.ne)
        assert len(idx) >= 32
        for x in (t, t0):
            x.inst.update_transition_matrices(idx, lens)
            for e in range(t.ne):
                x.edge(e).contents.l = float(lens[e])
        now, _, on_demand, _ = t.inst.deferred_stats()
        assert now == len(want) > 0 and on_demand == 0
        for k in keys:
            assert_reads_back(t, k, before[k])
        assert t.inst.deferred_stats()[2] == len(want)
        assert t.Lk(None) == t0.Lk(None)
    finally:
        t.close(); t0.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_both_sides_then_every_edge(shape):
    t, t0, ot = pair(shape)
    try:
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)
        for b in range(t.ne):
            assert t.Lk(b) == t0.Lk(b), b
        assert t.inst.deferred_stats()[0] == 0
        assert t.Lk(None) == t0.Lk(None)
        for k in ot.plk:
            assert_reads_back(t, k, (t0.partials(*k), t0.scale_factors(*k)))
    finally:
        t.close(); t0.close()
