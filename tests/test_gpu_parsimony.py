"""Parsimony on the device (phyml_amd/csrc/phyhip_pars.hip) against the reference's own integers (tests/golden/pars_<case>.npz) and
against the numpy restatement that test_parsimony_restatement.py holds to them (tests/pars_ref.py).  Every comparison is
np.array_equal on integers."""
import os

import numpy as np
import pytest

import pars_ref
from pars_ref import MAX_PARS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["nucleic_bionj", "nucleic_random1", "nucleic_random2", "proteic_bionj", "proteic_random1", "proteic_random2", "designed_nt",
         "designed_aa"]
_cache = {}


def fixture(case):
    if case not in _cache:
        _cache[case] = dict(np.load(os.path.join(HERE, "golden", "pars_%s.npz" % case)))
    return _cache[case]


def make_instance(masks, ns, nbuf, wght=None, **kw):
    from phyml_amd import capi
    n, P = masks.shape
    if "devices" not in kw:
        kw["device"] = 0
    inst = capi.Instance(n, nbuf, ns, P, 2 * n, 1, **kw)
    inst.set_pattern_weights(np.ones(P) if wght is None else wght)
    for t in range(n):
        inst.set_tip_partials(t, pars_ref.masks_to_partials(masks[t], ns))
    return inst


def random_masks(n, P, ns, seed):
    """seeded states with ambiguity codes: single states, the full set, and a handful of multi-state sets"""
    rng = np.random.RandomState(seed)
    full = (1 << ns) - 1
    sets = [1 << s for s in range(ns)] * 3 + [full, full] + [int(x) for x in rng.randint(1, full + 1, size=8)]
    return np.array(sets, np.int64)[rng.randint(len(sets), size=(n, P))]


def random_step(ns, seed):
    m = np.random.RandomState(seed).randint(1, 6, size=(ns, ns))
    np.fill_diagonal(m, 0)
    return m


def random_index(n, seed):
    el, er = pars_ref.random_tree(n, seed)
    v, b = pars_ref.neighbours(n, el, er)
    return pars_ref.TreeIndex(n, el, er, v, b)


def check_buffers(inst, pl, bufs, general, what):
    for b in bufs:
        if general:
            assert np.array_equal(inst.partial_parsimony(b, general=True), pl.get(b)), (what, b)
        else:
            ui, pars = inst.partial_parsimony(b)
            rui, rpars = pl.get(b)
            assert np.array_equal(ui, rui) and np.array_equal(pars, rpars), (what, b)


# ---- 1. the reference's dumps --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_fixture_through_the_c_abi(case, general):
    d = fixture(case)
    ns, T = int(d["ns"][0]), pars_ref.tree_of_fixture(d)
    inst = make_instance(pars_ref.char_masks(d["seq"], ns), ns, T.nbuf, d["wght"].astype(np.float64))
    try:
        inst.set_parsimony(general, d["step_mat"] if general else None)
        inst.update_partial_parsimony(T.both_sides())          # the both-sides traversal as ONE list
        ref = None if (not general or "ppars" in d) else pars_ref.Planes(pars_ref.char_masks(d["seq"], ns), ns, d["step_mat"]).run(T.both_sides())
        site_key, c_key = ("site_general", "cpars_general") if general else ("site_fitch", "cpars_fitch")
        for e in range(T.E):
            assert inst.edge_parsimony(T.left_idx[e], T.rght_idx[e]) == int(d[c_key][e]), (case, e)
            assert np.array_equal(inst.site_parsimony(), d[site_key][e]), (case, e)
            for s, b in ((0, T.left_idx[e]), (1, T.rght_idx[e])):
                if b < T.n:
                    continue
                if general:
                    want = d["ppars"][e][s] if ref is None else ref.get(b)
                    assert np.array_equal(inst.partial_parsimony(b, general=True), want), (case, e, s)
                else:
                    ui, pars = inst.partial_parsimony(b)
                    assert np.array_equal(ui, d["ui"][e][s]) and np.array_equal(pars, d["pars"][e][s]), (case, e, s)
    finally:
        inst.close()


def lk_tree(d, wght=None, **kw):
    """the C host layer's tree on a dumped topology, tips from the dumped characters through the host layer's own encoders"""
    import orc
    from phyml_amd import lktree, workloads
    n, ns, P = int(d["n_otu"][0]), int(d["ns"][0]), d["seq"].shape[1]
    blk = dict(workloads.model_block("model_gtr_g4" if ns == 4 else "model_lg_g4"))
    blk["ncatg"] = np.array([1.0]); blk["gamma_rr"] = np.array([1.0]); blk["gamma_r_proba"] = np.array([1.0])
    m = orc.Model(blk)
    t = lktree.LkTree(n, d["edge_left"], d["edge_rght"], np.full(2 * n - 3, 0.1), P, ns, 1, node_v=d["node_v"], node_b=d["node_b"], **kw)
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)
    t.Make_Tree_For_Lk(d["wght"].astype(np.float64) if wght is None else wght)
    t.set_tips(tip_chars=d["seq"])
    return t


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_fixture_through_the_host_layer(case, general):
    d = fixture(case)
    ns, T = int(d["ns"][0]), pars_ref.tree_of_fixture(d)
    t = lk_tree(d)
    try:
        # nucleotides: the host layer's own Get_Step_Mat; amino acids: the caller's table, here the one the reference wrote at run time
        t.Make_Tree_For_Pars(general, d["step_mat"] if (general and ns == 20) else None)
        if ns == 4:
            assert np.array_equal(t.step_mat, d["step_mat"])
        t.Set_Both_Sides(True)
        site_key, c_key = ("site_general", "cpars_general") if general else ("site_fitch", "cpars_fitch")
        e0 = int(d["node_b"][0][0])
        assert t.Pars(None) == int(d[c_key][e0]) == t.c_pars
        assert np.array_equal(t.site_pars, d[site_key][e0])
        for e in range(T.E):
            assert [t.side_buffer(e, 0), t.side_buffer(e, 1)] == [T.left_idx[e], T.rght_idx[e]]
            assert t.Pars(e) == int(d[c_key][e]), (case, e)
            assert np.array_equal(t.site_pars, d[site_key][e]), (case, e)
            for s in (0, 1):
                if (T.left_idx[e], T.rght_idx[e])[s] < T.n:
                    continue
                if not general:
                    ui, pars = t.Get_Partial_Pars(e, s)
                    assert np.array_equal(ui, d["ui"][e][s]) and np.array_equal(pars, d["pars"][e][s]), (case, e, s)
                elif "ppars" in d:
                    assert np.array_equal(t.Get_Partial_Pars(e, s), d["ppars"][e][s]), (case, e, s)
        # Update_Pars_At_Given_Edge: two queued operations and the score, one call
        assert t.Update_Pars_At_Given_Edge(T.E // 2) == int(d[c_key][T.E // 2])
    finally:
        t.close()


# ---- 2. ragged shapes against the restatement ------------------------------------------------------------------------------------------

def ragged_sizes():
    from phyml_amd import capi
    return [1, 2, 63, 64, 65, 127, 129, capi.PARS_TILE - 1, capi.PARS_TILE + 1, 3 * capi.PARS_TILE + 1]


@pytest.mark.parametrize("n", [3, 4, 17])
@pytest.mark.parametrize("ns", [4, 20])
def test_ragged_shapes(ns, n):
    T = random_index(n, 40 + n)
    ops = T.both_sides()
    inner = list(range(n, T.nbuf))
    for P in ragged_sizes():
        masks = random_masks(n, P, ns, 1000 * ns + 10 * n + P)
        w = np.random.RandomState(P).randint(0, 6, size=P).astype(np.float64)
        step = random_step(ns, P + n)
        inst = make_instance(masks, ns, T.nbuf, w)
        try:
            for general in (False, True):
                pl = pars_ref.Planes(masks, ns, step if general else None).run(ops)
                inst.set_parsimony(general, step if general else None)
                inst.update_partial_parsimony(ops)
                for e in sorted({0, T.E // 2, T.E - 1}):
                    site = pl.site_pars(T.left_idx[e], T.rght_idx[e])
                    assert inst.edge_parsimony(T.left_idx[e], T.rght_idx[e]) == pars_ref.weighted_sum(site, w), (ns, n, P, general, e)
                    assert np.array_equal(inst.site_parsimony(), site), (ns, n, P, general, e)
                check_buffers(inst, pl, inner, general, (ns, n, P))
        finally:
            inst.close()


# ---- 3. operation-list forms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("ns", [4, 20])
def test_operation_list_forms(ns, general):
    from phyml_amd import capi
    n, P, nbuf = 6, 131, 6 + 10
    masks = random_masks(n, P, ns, 77 + ns)
    w = np.random.RandomState(3).randint(1, 4, size=P).astype(np.float64)
    step = random_step(ns, 5) if general else None
    d = list(range(n, nbuf))
    forms = {
        "forwarded as child1": [(d[0], 0, 1), (d[1], d[0], 2)],                      # tip x tip, then inner x tip
        "forwarded as child2": [(d[2], 2, 3), (d[3], 4, d[2])],                      # tip x inner
        "missed then both": [(d[4], 0, 5), (d[5], 1, 2), (d[6], d[4], d[5]),          # inner x inner: child1 from memory, child2 forwarded
                             (d[7], d[6], d[6])],                                    # both children the previous result
        "one": [(d[8], d[7], 3)],
    }
    inst = make_instance(masks, ns, nbuf, w)
    try:
        inst.set_parsimony(general, step)
        pl = pars_ref.Planes(masks, ns, step)
        for what, ops in forms.items():
            pl.run(ops)
            inst.update_partial_parsimony(ops)
            b1, b2 = ops[-1][0], ops[0][0]
            assert inst.edge_parsimony(b1, b2) == pars_ref.weighted_sum(pl.site_pars(b1, b2), w), what
            assert np.array_equal(inst.site_parsimony(), pl.site_pars(b1, b2)), what
            check_buffers(inst, pl, [o[0] for o in ops], general, what)
        # a list of 0 operations: the score alone -- inner x inner, tip x inner, tip x tip
        for b1, b2 in ((d[6], d[3]), (2, d[8]), (d[1], 4), (0, 5)):
            assert inst.edge_parsimony(b1, b2) == pars_ref.weighted_sum(pl.site_pars(b1, b2), w), (b1, b2)
            assert np.array_equal(inst.site_parsimony(), pl.site_pars(b1, b2)), (b1, b2)
        # get_partial flushes the queue
        ops = [(d[9], d[8], d[0]), (d[0], d[9], 1)]
        pl.run(ops)
        inst.update_partial_parsimony(ops)
        check_buffers(inst, pl, [d[0], d[9]], general, "get flushes")
        # N single-operation calls followed by a score == one list
        ops = [(d[k % 4], d[(k - 1) % 4] if k else 0, k % n) for k in range(9)]
        for o in ops:
            inst.update_partial_parsimony([o])
        one_by_one = inst.edge_parsimony(d[0], d[1])
        site_a = inst.site_parsimony()
        bufs_a = [inst.partial_parsimony(b, general=general) for b in d[:4]]
        pl.run(ops)
        assert one_by_one == pars_ref.weighted_sum(pl.site_pars(d[0], d[1]), w) and np.array_equal(site_a, pl.site_pars(d[0], d[1]))
        check_buffers(inst, pl, d[:4], general, "one by one")
        # the same operations once more as one list, from the same state as far as they read it: run twice, compare with the restatement
        inst.update_partial_parsimony(ops)
        pl.run(ops)
        assert inst.edge_parsimony(d[0], d[1]) == pars_ref.weighted_sum(pl.site_pars(d[0], d[1]), w)
        check_buffers(inst, pl, d[:4], general, "one list")
        assert len(bufs_a) == 4
    finally:
        inst.close()


@pytest.mark.parametrize("general,ns", [(False, 4), (False, 20), (True, 4)])
def test_a_list_longer_than_the_staging_capacity(general, ns):
    """it crosses a flush: the operation behind the boundary reads the previous result from memory, not from registers"""
    from phyml_amd import capi
    n, P, nbuf = 5, 65, 5 + 3
    masks = random_masks(n, P, ns, 11)
    step = pars_ref.nt_step_mat() if general else None
    N = capi.PARS_STAGING + 7
    d = [n, n + 1, n + 2]
    ops = [(d[k % 3], d[(k - 1) % 3] if k else 0, k % n) for k in range(N)]
    inst = make_instance(masks, ns, nbuf)
    try:
        inst.set_parsimony(general, step)
        inst.update_partial_parsimony(ops)
        pl = pars_ref.Planes(masks, ns, step).run(ops)
        b1, b2 = d[(N - 1) % 3], d[(N - 2) % 3]
        assert inst.edge_parsimony(b1, b2) == pars_ref.weighted_sum(pl.site_pars(b1, b2), np.ones(P))
        check_buffers(inst, pl, d, general, "long list")
    finally:
        inst.close()


# ---- 4. weights ----------------------------------------------------------------------------------------------------------------------------

def test_weights():
    from phyml_amd import capi
    n, P, ns = 7, 300, 4
    T = random_index(n, 9)
    masks = random_masks(n, P, ns, 5)
    ops = T.both_sides()
    pl = pars_ref.Planes(masks, ns).run(ops)
    l, r = T.left_idx[1], T.rght_idx[1]
    site = pl.site_pars(l, r)
    assert site.sum() > 16
    inst = make_instance(masks, ns, T.nbuf, np.zeros(P))
    try:
        inst.set_parsimony(False)
        inst.update_partial_parsimony(ops)
        assert inst.edge_parsimony(l, r) == 0                         # zeros
        assert np.array_equal(inst.site_parsimony(), site)
        big = np.full(P, float(1 << 28))                              # the sum exceeds 2^31 (and 2^32): exact as a long long
        inst.set_pattern_weights(big)
        want = pars_ref.weighted_sum(site, big)
        assert want > (1 << 32)
        assert inst.edge_parsimony(l, r) == want                      # ... and the new weights are the ones used
        w3 = np.random.RandomState(1).randint(0, 1000, size=P).astype(np.float64)
        inst.set_pattern_weights(w3)
        assert inst.edge_parsimony(l, r) == pars_ref.weighted_sum(site, w3)
        w4 = w3.copy(); w4[P // 2] = 2.5                              # one weight that is no integer: refused, nothing runs
        inst.set_pattern_weights(w4)
        inst.update_partial_parsimony([(T.left_idx[0], 0, 1)])
        with pytest.raises(capi.PhyhipError) as ei:
            inst.edge_parsimony(l, r)
        assert ei.value.code == capi.ERROR_NO_IMPLEMENTATION
        assert inst.edge_parsimony(l, r, with_sum=False) is None      # the per-pattern scores alone need no weights
        pl.run([(T.left_idx[0], 0, 1)])
        assert np.array_equal(inst.site_parsimony(), pl.site_pars(l, r))
    finally:
        inst.close()


def test_host_layer_runs_the_truncating_loop_for_other_weights():
    d = fixture("designed_nt")
    P = d["seq"].shape[1]
    w = d["wght"].astype(np.float64) * 0.75 + 0.1
    t = lk_tree(d, wght=w)
    try:
        t.Make_Tree_For_Pars(False)
        t.Set_Both_Sides(True)
        e0 = int(d["node_b"][0][0])
        want = pars_ref.truncating_sum(d["site_fitch"][e0], w)
        assert want != int(d["cpars_fitch"][e0]) and len(w) == P
        assert t.Pars(None) == want == t.c_pars
        assert np.array_equal(t.site_pars, d["site_fitch"][e0])
    finally:
        t.close()


# ---- 5. tip rewrite ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("ns", [4, 20])
def test_tip_rewrite_is_seen(ns, general):
    n, P = 6, 200
    T = random_index(n, 3)
    masks = random_masks(n, P, ns, 21)
    step = random_step(ns, 2) if general else None
    ops = T.both_sides()
    inst = make_instance(masks, ns, T.nbuf)
    try:
        inst.set_parsimony(general, step)
        inst.update_partial_parsimony(ops)
        l, r = T.left_idx[0], T.rght_idx[0]
        pl = pars_ref.Planes(masks, ns, step).run(ops)
        assert inst.edge_parsimony(l, r) == pars_ref.weighted_sum(pl.site_pars(l, r), np.ones(P))
        m2 = masks.copy()
        for tip, pat, new in ((2, 5, (1 << (ns - 1)) | 1), (0, P - 1, 1 << 1), (5, 64, (1 << ns) - 1)):   # the first: a state set not seen before
            m2[tip, pat] = new
            inst.set_tip_partials_at_pattern(tip, pat, pars_ref.masks_to_partials(m2[tip, pat:pat + 1], ns)[0])
        inst.update_partial_parsimony(ops)
        pl2 = pars_ref.Planes(m2, ns, step).run(ops)
        assert not np.array_equal(pl2.site_pars(l, r), pl.site_pars(l, r))
        assert inst.edge_parsimony(l, r) == pars_ref.weighted_sum(pl2.site_pars(l, r), np.ones(P))
        assert np.array_equal(inst.site_parsimony(), pl2.site_pars(l, r))
        check_buffers(inst, pl2, range(n, T.nbuf), general, "after the rewrite")
    finally:
        inst.close()


# ---- 6. sharded instances ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general,ns", [(False, 4), (True, 20)])
def test_sharded_instances(general, ns):
    n, P = 8, 2 * 256 + 77
    T = random_index(n, 12)
    masks = random_masks(n, P, ns, 31)
    w = np.random.RandomState(8).randint(0, 50, size=P).astype(np.float64)
    step = random_step(ns, 9) if general else None
    ops = T.both_sides()
    pl = pars_ref.Planes(masks, ns, step).run(ops)
    l, r = T.left_idx[2], T.rght_idx[2]
    for shards in (1, 2, 3):
        inst = make_instance(masks, ns, T.nbuf, w, devices=[0] * shards, force_sharded=True)
        try:
            inst.set_parsimony(general, step)
            inst.update_partial_parsimony(ops)
            assert inst.edge_parsimony(l, r) == pars_ref.weighted_sum(pl.site_pars(l, r), w), shards
            assert np.array_equal(inst.site_parsimony(), pl.site_pars(l, r)), shards
            check_buffers(inst, pl, range(n, T.nbuf), general, shards)
        finally:
            inst.close()


# ---- 7. mode switch ------------------------------------------------------------------------------------------------------------------------

def test_mode_switch():
    n, P, ns = 6, 150, 4
    T = random_index(n, 4)
    masks = random_masks(n, P, ns, 6)
    ops, step = T.both_sides(), random_step(ns, 1)
    l, r = T.left_idx[3], T.rght_idx[3]
    inst = make_instance(masks, ns, T.nbuf)
    try:
        for general in (False, True, False):
            inst.set_parsimony(general, step if general else None)
            inst.update_partial_parsimony(ops)
            pl = pars_ref.Planes(masks, ns, step if general else None).run(ops)
            assert inst.edge_parsimony(l, r) == int(pl.site_pars(l, r).sum())
            check_buffers(inst, pl, range(n, T.nbuf), general, general)
    finally:
        inst.close()


# ---- 8. isolation --------------------------------------------------------------------------------------------------------------------------

def _likelihood_run(with_parsimony):
    from gpu_common import synthetic_pair
    t, ot, tree, st = synthetic_pair(26, 150, 4, 4, seed=6, ambiguous_every=6)
    try:
        t.Set_Both_Sides(True)
        first = t.Lk(None)
        b5 = t.Lk(5)
        if with_parsimony:
            t.Make_Tree_For_Pars(False)
            t.Set_Both_Sides(True)
            t.Pars(None)
        t.Update_All_Partial_Lk()                      # likelihood operations queued and not launched
        stats = t.inst.virtual_stats()
        if with_parsimony:
            c = t.Pars(None)
            assert t.Update_Pars_At_Given_Edge(7) == c
            t.Get_Partial_Pars(7, 0)
            t.Make_Tree_For_Pars(True)
            t.Pars(None)
            t.inst.profile_read_parsimony()
            assert t.inst.virtual_stats() == stats     # ... stay queued: no traversal launch has happened
        lnl = t.Lk(None)
        return first, b5, lnl, t.inst.site_outputs(), t.inst.numerical_warning(), t.Lk(9)
    finally:
        t.close()


def test_isolation_from_the_likelihood_surface():
    a, b = _likelihood_run(False), _likelihood_run(True)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[5] == b[5]      # bit-equal doubles
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    assert a[4] == b[4]


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------------

def _code(fn, *args, **kw):
    from phyml_amd import capi
    with pytest.raises(capi.PhyhipError) as ei:
        fn(*args, **kw)
    return ei.value.code


def test_errors():
    from phyml_amd import capi
    n, P, ns = 4, 20, 4
    masks = random_masks(n, P, ns, 1)
    inst = make_instance(masks, ns, n + 4)
    try:
        for fn, args in ((inst.update_partial_parsimony, ([(n, 0, 1)],)), (inst.edge_parsimony, (0, 1)), (inst.site_parsimony, ()),
                         (inst.partial_parsimony, (n,)), (inst.profile_read_parsimony, ())):
            assert _code(fn, *args) == capi.ERROR_UNINITIALIZED_INSTANCE, fn
        assert _code(inst.set_parsimony, True, None) == capi.ERROR_OUT_OF_RANGE              # the step-matrix mode without a matrix
        inst.set_parsimony(False)
        for op in ((n + 4, 0, 1), (-1, 0, 1), (n, n + 4, 1), (n, 0, -1),                     # out of range
                   (1, 0, 2),                                                                # a destination that is a tip
                   (n, n, 1), (n + 1, 0, n + 1)):                                            # a destination that is one of its children
            assert _code(inst.update_partial_parsimony, [(n + 1, 0, 1), op]) == capi.ERROR_OUT_OF_RANGE, op
        assert _code(inst.edge_parsimony, 0, n + 4) == capi.ERROR_OUT_OF_RANGE
        assert _code(inst.partial_parsimony, 1) == capi.ERROR_OUT_OF_RANGE
        assert _code(inst.partial_parsimony, n, general=True) == capi.ERROR_OUT_OF_RANGE     # the Fitch mode holds no p_pars
        # nothing of the refused lists was queued: the plane is what a fresh one is
        inst.update_partial_parsimony([(n, 0, 1)])
        pl = pars_ref.Planes(masks, ns).run([(n, 0, 1)])
        assert inst.edge_parsimony(n, 2) == int(pl.site_pars(n, 2).sum())
    finally:
        inst.close()
    cls = capi.Instance(4, 10, 4, 16, 5, 4, device=0, class_axis=True)
    try:
        assert _code(cls.set_parsimony, False) == capi.ERROR_NO_IMPLEMENTATION
        assert _code(cls.edge_parsimony, 0, 1) == capi.ERROR_NO_IMPLEMENTATION
    finally:
        cls.close()
    rank = make_instance(masks, ns, n + 4)
    try:
        rank.comm_init_rank(1, 0, capi.comm_get_unique_id())
        assert _code(rank.set_parsimony, False) == capi.ERROR_NO_IMPLEMENTATION
    finally:
        rank.close()


def test_profile_counts_the_launches():
    n, P, ns = 5, 300, 4
    T = random_index(n, 2)
    inst = make_instance(random_masks(n, P, ns, 2), ns, T.nbuf)
    try:
        inst.set_parsimony(False)
        inst.profile(1)
        inst.update_partial_parsimony(T.both_sides())
        inst.edge_parsimony(T.left_idx[0], T.rght_idx[0])
        inst.edge_parsimony(T.left_idx[1], T.rght_idx[1])
        ms, launches, updates = inst.profile_read_parsimony()
        assert launches == 2 and ms > 0.0 and updates == P * (len(T.both_sides()) + 2)
        assert inst.profile_read_parsimony() == (0.0, 0, 0.0)
        inst.profile(0)
    finally:
        inst.close()
