"""Compact step records of the nucleotide list form (phyml_amd/csrc/phyhip_kernels.hpp: NtIssue / NtExec; built by
fill_compact_records, phyhip_queue.hip; read by nt2_run with ARGS == 0, phyhip_nt2.hpp; profiles/r13_nt_records.md).  A child or a
destination is a 32-bit offset in 16-byte units from the base of its arena and a flag bit says whether it is loaded or stored at
all, so what can go wrong is an offset (a wrong buffer, a wrong row of the scale or tip table), a flag (a load or a store that
is skipped, or not), the in-step child's packed fields, and the record consumed one step off -- each shows in some internal
partial vector or scale vector.

Check, through the C ABI: after Lk(NULL) EVERY internal partial vector and scale vector is np.array_equal to the oracle's
(tests/orc.py) and lnL agrees with it, at the shapes of tests/test_gpu_nt_chain.py -- the smallest that reach each list-form
kernel and both parities of the list length -- in three store settings (default; every operation stores; chained buffers off)
and both traversal forms (the pre-order half of a both-sided traversal loads stored children from all over the arena)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_common import device_compute_units, synthetic_oracle
from phyml_amd import lktree, synth
from test_gpu_nt_chain import ambiguous_oracle, device_tree, written


@functools.lru_cache(maxsize=None)
def mixed_patterns():
    """both wave shapes in one launch: one full round of two-lane workgroups (32 patterns each) and a four-lane rest"""
    return 32 * device_compute_units() + 38


def shapes():
    return [(300, 96, 7, False), (301, 96, 7, False), (40, "mixed", 3, False), (40, "mixed", 3, True), (20, 131200, 5, False)]


def patterns(P):
    return mixed_patterns() if P == "mixed" else P


@functools.lru_cache(maxsize=None)
def reference(n_otu, P, seed, ambiguous, both):
    """(oracle tree after Lk(NULL) one- or both-sided, its lnL, random tree, tip vectors, weights): once per shape, read-only"""
    if ambiguous:
        ot, tree, tv, wg = ambiguous_oracle(n_otu, P, seed)
    else:
        ot, tree, _, tv, wg = synthetic_oracle(n_otu, P, 4, 4, seed)
    return ot, ot.lk(None, both_sides=both), tree, tv, wg


SETTINGS = ["default", "all_stored", "unchained"]


def configure(t, setting, both):
    if setting == "all_stored":
        t.inst.set_virtual_buffers(0)
    elif setting == "unchained":
        t.inst.set_chained_buffers(0)
    t.Set_Both_Sides(both)


@pytest.mark.parametrize("both", [False, True], ids=["one_sided", "both_sided"])
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("n_otu,P,seed,ambiguous", shapes())
def test_every_internal_buffer_is_the_oracles(n_otu, P, seed, ambiguous, setting, both):
    P = patterns(P)
    ot, ref, tree, tv, wg = reference(n_otu, P, seed, ambiguous, both)
    t = device_tree(ot, tree, tv, wg, P)
    try:
        configure(t, setting, both)
        lnl = t.Lk(None)
        st = t.inst.record_stats()
        print(f"{n_otu} x {P} {setting} both={both}: lnL {lnl!r} oracle {ref!r} records {st} virtual {t.inst.virtual_stats()} "
              f"chained {t.inst.chained_stats()}")
        assert st[0] >= 1 and st[1] == 0            # the launch read a compact list, built for it
        assert abs(lnl - ref) / abs(ref) < 1e-12
        if setting == "all_stored":
            assert t.inst.virtual_stats() == (0, 0, 0, 0) and t.inst.chained_stats()[0] == 0 and st[2 + 1] == st[7 + 1] == 0
        elif setting == "unchained":
            assert t.inst.chained_stats()[0] == 0
        elif not both and n_otu >= 40:
            # (a one-sided traversal chains, a both-sided one never does; the 20-taxon list, 18 operations less its 5 in-step
            # children, is below the 16 operations chaining starts at)
            assert t.inst.chained_stats()[0] > 0
        if setting != "all_stored":
            assert t.inst.virtual_stats()[0] > 0 and st[2 + 1] + st[7 + 1] > 0   # in-step children
        keys = list(ot.plk) if both else written(ot)
        assert len(keys) >= n_otu - 2
        for k in keys:   # (reading an unstored buffer stores its definition first: a launch of its own with stored definitions in front)
            assert np.array_equal(t.partials(*k), ot.plk[k]), k
            assert np.array_equal(t.scale_factors(*k), ot.scale[k]), k
        assert t.Lk(None) == lnl
    finally:
        t.close()


KINDS = ("tip", "in-step", "forwarded k-1", "forwarded k-2", "loaded")


def test_the_chosen_trees_have_every_child_kind_in_both_positions():
    """What the equality above covers, said by the host that built the lists: over a default one-sided and a default both-sided
    traversal, every kind of child -- a tip row, a virtual tip x tip result computed in the step, a result forwarded from the
    previous or the second-previous operation, a stored buffer -- occurs as the first and as the second child of some operation of
    the 300- and 301-taxon trees, and over all the trees together."""
    total = np.zeros(10, dtype=np.int64)
    for (n_otu, P, seed, ambiguous) in shapes():
        P = patterns(P)
        per_tree = np.zeros(10, dtype=np.int64)
        for both in (False, True):
            ot, _, tree, tv, wg = reference(n_otu, P, seed, ambiguous, both)
            t = device_tree(ot, tree, tv, wg, P)
            try:
                t.Set_Both_Sides(both)
                t.Lk(None)
                per_tree += np.array(t.inst.record_stats()[2:], dtype=np.int64)
            finally:
                t.close()
        print(f"{n_otu} x {P}: child 1 {dict(zip(KINDS, per_tree[:5]))} child 2 {dict(zip(KINDS, per_tree[5:]))}")
        if n_otu >= 300:
            assert (per_tree > 0).all(), per_tree
        total += per_tree
    assert (total > 0).all(), total


def test_an_edge_evaluation_behind_a_one_sided_traversal_stores_definitions_in_front_of_a_list():
    """Lk(b) at an inner edge behind a one-sided traversal: the sides of b are chained or deferred, so their definitions -- and
    what those read -- are stored in front of the evaluation, in ONE list-form launch that loads, forwards and stores all over
    the arena.  Against the oracle's Lk(b)."""
    n_otu, P, seed = 40, mixed_patterns(), 3
    _, _, tree, tv, wg = reference(n_otu, P, seed, False, True)
    ot = synthetic_oracle(n_otu, P, 4, 4, seed)[0]   # (an oracle of its own: its state follows the calls below)
    t = device_tree(ot, tree, tv, wg, P)
    try:
        t.Set_Both_Sides(True)
        ref0 = ot.lk(None, both_sides=True)
        assert abs(t.Lk(None) - ref0) / abs(ref0) < 1e-12   # every buffer written once
        t.Set_Both_Sides(False)
        inner = [e for e in range(t.ne) if ot.el[e] >= ot.n and ot.er[e] >= ot.n]
        stored_lists = 0
        for e in inner[::3]:
            lnl1, ref1 = t.Lk(None), ot.lk(None)
            assert abs(lnl1 - ref1) / abs(ref1) < 1e-12
            assert t.inst.chained_stats()[0] > 0
            before_c, before_r = t.inst.chained_stats()[2], t.inst.record_stats()[0]
            lnl, ref = t.Lk(e), ot.lk(e)
            on_demand, lists = t.inst.chained_stats()[2] - before_c, t.inst.record_stats()[0] - before_r
            print(f"edge {e}: lnL {lnl!r} oracle {ref!r}; {on_demand} chained definitions stored, {lists} compact lists built")
            assert abs(lnl - ref) / abs(ref) < 1e-12, e
            stored_lists += int(on_demand > 0 and lists > 0)
        assert stored_lists > 0
    finally:
        t.close()


def test_a_repeated_traversal_reuses_its_slot_and_another_list_does_not():
    n_otu, P, seed = 300, 96, 7
    ot, _, tree, tv, wg = reference(n_otu, P, seed, False, False)
    ot2 = synthetic_oracle(n_otu, P, 4, 4, seed)[0]
    t = device_tree(ot, tree, tv, wg, P)
    try:
        lnl = t.Lk(None)
        assert t.inst.record_stats()[:2] == (1, 0)
        assert t.Lk(None) == lnl and t.Lk(None) == lnl
        assert t.inst.record_stats()[:2] == (1, 2)      # the same list twice more: nothing built, nothing uploaded
        # the traversal from another tip is another list over the same buffers: built, not taken from the slot
        other = int(t.tip_root) + 1
        t.tip_root = other; ot2.tip_root = other
        lnl2, ref2 = t.Lk(None), ot2.lk(None)
        built, reused = t.inst.record_stats()[:2]
        print("records after the second list:", (built, reused))
        assert built >= 2 and reused == 2
        assert abs(lnl2 - ref2) / abs(ref2) < 1e-12
        for k in written(ot2):
            assert np.array_equal(t.partials(*k), ot2.plk[k]), k
            assert np.array_equal(t.scale_factors(*k), ot2.scale[k]), k
    finally:
        t.close()


def test_offsets_beyond_four_gib():
    """An instance whose partials arena is larger than 2^32 bytes: a both-sided traversal writes and reads buffers whose offset
    from the arena's base does not fit 32 bits of BYTES (the records count 16-byte units).  No oracle run at this size: lnL
    against the same data on two shards (each arena below 4 GiB; the block sums are partitioned differently) and against the
    exact-site route's ordered sum at the root edge, 1e-12 relative."""
    P = 131072
    buf_bytes = P * 4 * 4 * 8
    n_otu = 2
    while (3 * n_otu - 6) * buf_bytes <= (1 << 32) + 4 * buf_bytes:   # internal edge sides of an unrooted tree: 3 n - 6
        n_otu += 1
    m = synthetic_oracle(4, 8, 4, 4, 9)[0].m
    tree = synth.random_tree(n_otu, 9, 0.02, 0.3)
    st = synth.simulate_states(tree, P, 4, 9)
    tv = [np.eye(4)[st[k]] for k in range(n_otu)]
    wg = np.ones(P)

    def make(devices):
        t = lktree.LkTree(n_otu, tree.edge_left, tree.edge_rght, tree.edge_len, P, 4, 4, host_pmat=True, devices=devices,
                          force_sharded=devices is not None)
        t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)
        t.Make_Tree_For_Lk(wg)
        t.set_tips(tip_partials=tv)
        t.Set_Both_Sides(True)
        return t

    t = make(None)
    try:
        lnl = t.Lk(None)
        exact = t.Exact_Site_Lk(None)[0]
        again = t.Lk(None)
    finally:
        t.close()
    t2 = make((0, 0))
    try:
        lnl2 = t2.Lk(None)
    finally:
        t2.close()
    print(f"{n_otu} taxa x {P}: arena {(3 * n_otu - 6) * buf_bytes / 2**30:.2f} GiB, lnL {lnl!r} two shards {lnl2!r} exact {exact!r}")
    assert again == lnl
    assert abs(lnl - lnl2) / abs(lnl) < 1e-12
    assert abs(lnl - exact) / abs(lnl) < 1e-12
