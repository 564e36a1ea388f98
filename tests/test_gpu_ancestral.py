"""phyhip_calculate_node_state_posteriors (phyml_amd/csrc/phyhip_ancestral.hip; Get_Ancestral_Probs / Get_All_Ancestral_Probs in the
host layer): the marginal state posteriors of internal nodes on the device, against the numpy restatement of
Ancestral_Sequences_One_Node (tests/ancestral_ref.py, itself held to the reference's printed output by
tests/test_ancestral_restatement.py) and against the reference's own files.

Device against restatement: 1e-10 relative per entry with a 1e-300 floor -- the project's per-site gate.  Every term is
non-negative, so nothing cancels: (3S + C + 4) 2^-53 before the log plus 2^-53 (|log q| + LOG2 ss + |lnL_p|) through log / exp is
under 1e-12 at these sizes.  To compare arithmetic only, both sides get the same site log-likelihoods: the oracle tree's own passed
in, or NULL on the device and the device's own phyhip_get_site_log_likelihoods given to the restatement.  No bit parity with the
reference's binary is claimed for this call; equalities between two DEVICE results (batching, sharding, virtual buffers, the host
layer) are np.array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ancestral_ref as ar
import orc
from conftest import FIXTURES
from gpu_common import assert_device_state_is_the_oracles, device_tree_from_golden, synthetic_oracle, synthetic_pair
from phyml_amd import capi, lktree

TOL, FLOOR = 1e-10, 1e-300
PRINT_TOL = 5.1e-6   # %10g: 6 significant digits (5e-6) + the arithmetic (tests/test_ancestral_restatement.py)
SMALL_SHAPES = {4: (9, 300), 20: (7, 270)}   # cross a 256-lane workgroup, ragged tail, Ppad != P in the fragment-major layout
SEED = 3                                     # both trees have nodes with 0, 1 and 2 tip neighbours (asserted below)


def indices(t, ot, nodes=None):
    """The three (side buffer or tip, matrix) pairs per node, resolved by hand from the oracle tree's adjacency (src/ancestral.c:661-706)"""
    nodes = ar.internal_nodes(ot) if nodes is None else nodes
    sides = [[v if v < ot.n else t.side_buffer(be, side) for (v, be, side) in ar.node_sides(ot, d)] for d in nodes]
    mats = [[t.edge(be).contents.Pij_rr_idx for (_, be, _) in ar.node_sides(ot, d)] for d in nodes]
    return np.array(sides, np.int32).reshape(-1, 3), np.array(mats, np.int32).reshape(-1, 3)


def assert_close(got, ref, what=None):
    err = np.abs(got - ref)
    bound = TOL * np.maximum(np.abs(ref), FLOOR)
    worst = float(np.max(err / np.maximum(np.abs(ref), FLOOR))) if err.size else 0.0
    print(what, "worst relative difference:", worst)
    assert np.all(err <= bound), (what, worst)


def assert_both_forms(t, ot, what=None):
    """All internal nodes in one call, the site log-likelihoods passed in and read on the device; rows without weight are zero."""
    sides, mats = indices(t, ot)
    w = ot.wght > 0
    got, warn = t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted, with_warning=True)
    assert_close(got, ar.node_posteriors(ot)[0], (what, "site lnL passed in"))
    assert warn == 0 and not np.any(got[:, ~w])
    dev_lnl = t.inst.site_log_likelihoods()
    got2 = t.inst.node_state_posteriors(sides, mats)
    assert_close(got2, ar.node_posteriors(ot, site_lnl=dev_lnl)[0], (what, "site lnL read on the device"))
    assert not np.any(got2[:, ~w])
    assert np.all(np.abs(got2[:, w].sum(axis=2) - 1.0) <= 1e-6)
    return got, got2


@pytest.fixture(scope="module")
def evaluated(golden):
    """Per fixture: device tree and restatement after Lk(NULL) with both sides set (every partial vector current), shared."""
    cache = {}

    def get(name):
        if name not in cache:
            d = golden(name)
            t, ot = device_tree_from_golden(d)
            t.Set_Both_Sides(True)
            t.Lk(None)
            ot.lk(None, both_sides=True)
            cache[name] = (d, t, ot)
        return cache[name]
    yield get
    for v in cache.values():
        v[1].close()


@pytest.fixture(scope="module")
def small():
    """The smallest shapes that can still go wrong (4 categories, uploaded matrices), evaluated, shared and left unchanged."""
    cache = {}

    def get(ns):
        if ns not in cache:
            n, P = SMALL_SHAPES[ns]
            t, ot, tree, st = synthetic_pair(n, P, ns, 4, seed=SEED, ambiguous_every=5)
            t.Set_Both_Sides(True)
            t.Lk(None)
            ot.lk(None, both_sides=True)
            sides, mats = indices(t, ot)
            cache[ns] = (t, ot, sides, mats, t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted))
        return cache[ns]
    yield get
    for v in cache.values():
        v[0].close()


# golden fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures(name, evaluated):
    d, t, ot = evaluated(name)
    assert_both_forms(t, ot, name)
    if name == "nucleic_zero_w":
        assert int((ot.wght > 0).sum()) >= 300 and np.any(ot.wght == 0)


@pytest.mark.parametrize("name,shape", [("synth_nt_300x40", (300, 40, 4)), ("synth_aa_90x24", (90, 24, 20))])
def test_reference_files(name, shape, evaluated):
    """The device result against what the real reference printed for the same tree (tests/golden/make_ancestral.py)."""
    d, t, ot = evaluated(name)
    ref, seen = ar.load_reference_file(name, *shape)
    assert len(seen) == (shape[0] - 2) * shape[1]
    got = t.Ancestral_Probs()
    err = np.abs(got - ref)
    print(name, "worst relative difference to the printed value:", float(np.max(err / np.maximum(np.abs(ref), FLOOR))))
    assert np.all(err <= PRINT_TOL * np.abs(ref))


# smallest shapes that can still go wrong ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_pmat", [True, False])
@pytest.mark.parametrize("Cc", [1, 4, 5, 8, 33, 64])
@pytest.mark.parametrize("ns", [4, 20])
def test_small_shapes(ns, Cc, host_pmat):
    n, P = SMALL_SHAPES[ns]
    t, ot, tree, st = synthetic_pair(n, P, ns, Cc, seed=SEED, host_pmat=host_pmat, ambiguous_every=5)
    try:
        tips_at = sorted({sum(v < ot.n for (v, _, _) in ar.node_sides(ot, d)) for d in ar.internal_nodes(ot)})
        assert tips_at == [0, 1, 2], tips_at
        assert any(a.any() for a in ot.tip_amb)
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        assert_both_forms(t, ot, (ns, Cc, host_pmat))
    finally:
        t.close()


# node indexing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_node_indexing(ns, small):
    t, ot, sides, mats, batched = small(ns)
    for k in range(len(sides)):
        one = t.inst.node_state_posteriors(sides[k:k + 1], mats[k:k + 1], ot.c_lnL_sorted)
        assert np.array_equal(one[0], batched[k]), k
    rev = t.inst.node_state_posteriors(sides[::-1], mats[::-1], ot.c_lnL_sorted)
    assert np.array_equal(rev, batched[::-1])
    assert np.array_equal(t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted), batched)   # (the kept work space, used again)


# sharding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_sharded_group_returns_the_unsharded_doubles(ns, small):
    t1, ot, sides, mats, ref = small(ns)
    n, P = SMALL_SHAPES[ns]
    t, _, _, _ = synthetic_pair(n, P, ns, 4, seed=SEED, ambiguous_every=5, devices=[0, 0, 0], force_sharded=True)
    try:
        assert len(t.inst.shard_ranges()) == 3
        t.Set_Both_Sides(True)
        t.Lk(None)
        s2, m2 = indices(t, ot)
        assert np.array_equal(s2, sides) and np.array_equal(m2, mats)
        assert np.array_equal(t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted), ref)
        assert np.array_equal(t.inst.node_state_posteriors(sides[2:3], mats[2:3], ot.c_lnL_sorted)[0], ref[2])
        got = t.inst.node_state_posteriors(sides, mats)   # each shard reads its own range of the last evaluation's site lnL
        assert_close(got, ar.node_posteriors(ot, site_lnl=t.inst.site_log_likelihoods())[0], (ns, "sharded, site lnL on the device"))
    finally:
        t.close()


# virtual buffers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,P", [(4, 150), (20, 40)])
def test_virtual_buffers_are_stored_for_the_call(ns, P):
    """A whole-tree traversal of more than 16 operations leaves its tip x tip results virtual.  The call made straight after it,
    and the call made with the whole traversal queued again and not yet launched, return what an instance that never leaves a
    buffer virtual returns."""
    got = {}
    for virtual in (True, False):
        t, ot, tree, st = synthetic_pair(26, P, ns, 4, seed=6, host_pmat=True, ambiguous_every=6)
        try:
            if not virtual:
                t.inst.set_virtual_buffers(0)
            t.Set_Both_Sides(True)
            t.Lk(None)
            ot.lk(None, both_sides=True)
            now = t.inst.virtual_stats()[0]
            assert (now > 0) == virtual
            sides, mats = indices(t, ot)
            a = t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted)
            if virtual:
                assert t.inst.virtual_stats()[0] < now and t.inst.virtual_stats()[3] > 0
            t.Update_All_Partial_Lk()   # queued, not launched
            b = t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted)
            got[virtual] = (a, b)
            assert_close(a, ar.node_posteriors(ot)[0], (ns, virtual))
        finally:
            t.close()
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(got[True][1], got[False][1])
    assert np.array_equal(got[True][0], got[True][1])


# +I: Invariant_Lk's overflow branch ---------------------------------------------------------------------------------------------
def invariant_pair(n, P, ns, Cc, seed, pinvar):
    """synthetic_pair with a +I model: invar[p] = the state every tip shows at p, else -1 (tree->data->invar)"""
    ot0, tree, st, tv, wg = synthetic_oracle(n, P, ns, Cc, seed)
    invar = np.where((st == st[0]).all(axis=0), st[0].astype(np.int16), np.int16(-1)).astype(np.int16)
    m = ot0.m
    m.invar_model, m.pinvar = 1, pinvar
    ot = orc.OracleTree(m, n, tree.edge_left, tree.edge_rght, tree.edge_len, wg, ot0.tip_vec, ot0.tip_ds, ot0.tip_amb, invar=invar)
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, ns, Cc, host_pmat=True)
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1, 1, pinvar)
    t.Make_Tree_For_Lk(wg, invar)
    t.set_tips(tip_partials=tv)
    return t, ot


@pytest.mark.parametrize("ns", [4, 20])
def test_invariant_overflow_branch(ns):
    n, P = SMALL_SHAPES[ns]
    t, ot = invariant_pair(n, 70, ns, 4, SEED, 0.2)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        assert int((ot.invar >= 0).sum()) >= 3 and np.any(ot.invar < 0)
        assert_both_forms(t, ot, (ns, "+I"))   # (warning 0)
        d = next(d for d in ar.internal_nodes(ot) if all(v >= ot.n for (v, _, _) in ar.node_sides(ot, d)))
        p0 = int(np.flatnonzero(ot.invar >= 0)[1])
        lift = 400   # three sides: ss >= 1200, pi x 2^1200 is infinite
        for (v, be, side) in ar.node_sides(ot, d):
            buf = t.side_buffer(be, side)
            s = t.inst.get_scale_factors(buf)
            assert np.array_equal(s, ot.scale[(be, side)])
            s[p0] += lift
            capi._chk(t.inst.L.phyhip_set_scale_factors(t.inst.id, buf, capi._ptr(s)))
            ot.scale[(be, side)][p0] += lift
        # (site log-likelihoods passed in, lowered at p0 by part of what the lift took: e^-232 at this node, e^600 at the other
        # nodes -- every entry stays a finite normal double, so that the comparison says something)
        lnl = ot.c_lnL_sorted.copy()
        lnl[p0] -= 600.0
        ref, ref_warn = ar.node_posteriors(ot, site_lnl=lnl)
        assert ref_warn == 1
        sides, mats = indices(t, ot)
        got, warn = t.inst.node_state_posteriors(sides, mats, lnl, with_warning=True)
        assert warn == 1
        assert_close(got, ref, (ns, "+I overflow"))
        k = ar.internal_nodes(ot).index(d)
        assert np.all(np.isfinite(ref)) and np.all(ref[k, p0] > 1e-200) and np.all(got[k, p0] > 1e-200)
        # the node alone raises it, another node alone does not
        assert t.inst.node_state_posteriors(sides[k:k + 1], mats[k:k + 1], lnl, with_warning=True)[1] == 1
        other = next(j for j in range(len(sides)) if j != k and not set(sides[j]) & set(sides[k]))
        assert t.inst.node_state_posteriors(sides[other:other + 1], mats[other:other + 1], lnl, with_warning=True)[1] == 0
    finally:
        t.close()


# nothing else moves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nucleic_gtr_g4_inv", "proteic_lg_g4"])
def test_nothing_else_moves(name, golden):
    """What the hot path left and what it returns next are the same doubles with and without the call in between."""
    d = golden(name)
    seen = []
    for with_call in (False, True):
        t, ot = device_tree_from_golden(d)
        try:
            t.Set_Both_Sides(True)
            lnl = t.Lk(None)
            ot.lk(None, both_sides=True)
            if with_call:
                t.Ancestral_Probs()
                t.Ancestral_Probs(ot.n + 3)
            out = t.inst.site_outputs()
            warn = t.inst.numerical_warning()
            if with_call:
                sides, mats = indices(t, ot)
                t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted)
                assert_device_state_is_the_oracles(t, ot, what=name)
            seen.append((lnl, out, warn, t.Lk(5), t.Lk(7)))
        finally:
            t.close()
    (l0, o0, w0, a0, b0), (l1, o1, w1, a1, b1) = seen
    assert l0 == l1 and w0 == w1 and a0 == a1 and b0 == b1
    for x, y in zip(o0, o1):
        assert np.array_equal(x, y)


# errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors(golden, small):
    inst = capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True)
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            inst.node_state_posteriors([[4, 5, 0]], [[0, 1, 2]])
    finally:
        inst.close()
    t, ot = device_tree_from_golden(golden("nucleic_gtr_g4"), use_m4mod=True, arith=2)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        sides, mats = indices(t, ot)
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            t.inst.node_state_posteriors(sides, mats)
        with pytest.raises(capi.PhyhipError, match="generic-loop"):
            t.Ancestral_Probs()
    finally:
        t.close()
    t, ot, sides, mats, ref = small(4)
    nbuf = ot.n + len(ot.plk) + 64
    for bad in (-1, nbuf):
        s = sides.copy(); s[2, 1] = bad
        with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
            t.inst.node_state_posteriors(s, mats)
    for bad in (-1, t.inst.nmat + 64):
        m = mats.copy(); m[1, 2] = bad
        with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
            t.inst.node_state_posteriors(sides, m)
    empty = t.inst.node_state_posteriors(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
    assert empty.shape == (0, ot.P, 4)
    assert np.array_equal(t.inst.node_state_posteriors(sides, mats, ot.c_lnL_sorted), ref)   # the errors left nothing behind


# host layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_host_layer(ns, small):
    t, ot, sides, mats, _ = small(ns)
    all_nodes = t.Ancestral_Probs()
    assert all_nodes.shape == (ot.n - 2, ot.P, ns)
    assert np.array_equal(all_nodes, t.inst.node_state_posteriors(sides, mats))
    for k in (0, 3, ot.n - 3):
        assert np.array_equal(t.Ancestral_Probs(ot.n + k), all_nodes[k]), k
    with pytest.raises(capi.PhyhipError, match="tip"):
        t.Ancestral_Probs(0)


def test_host_layer_exit_handler_when_the_site_lnl_is_another_trees():
    """Lk(b) after one edge length changed, the partials not refreshed: the site log-likelihoods on the device now belong to
    another state of the tree than the partials a node reads, its probabilities no longer sum to 1 and the reference's check
    (src/ancestral.c:878-885) fires."""
    t, ot, tree, st = synthetic_pair(9, 300, 4, 4, seed=SEED, ambiguous_every=5)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        t.Ancestral_Probs()   # in step: passes
        b = 5
        d = next(d for d in ar.internal_nodes(ot) if all(be != b for (_, be, _) in ar.node_sides(ot, d)))
        ot.len[b] = 25.0 * ot.len[b] + 2.0
        ot.lk(b)
        sums = ar.node_posteriors(ot, [d])[0][0].sum(axis=1)
        assert np.any(np.abs(sums[ot.wght > 0] - 1.0) >= 0.01)   # the restatement leaves the band first
        t.edge(b).contents.l = float(ot.len[b])
        t.Lk(b)
        with pytest.raises(capi.PhyhipError, match="Probabilities do not sum to 1.0"):
            t.Ancestral_Probs(d)
        with pytest.raises(capi.PhyhipError, match="Probabilities do not sum to 1.0"):
            t.Ancestral_Probs()
    finally:
        t.close()
