"""The host layer the calls beside the hot path share (phyml_amd/csrc/phyhip_side.hpp) -- work spaces that grow between two calls
of one instance, the per-shard profile sums, and parsimony entered as a query while resident workgroups serve -- held to what a
fresh instance answers, bit for bit.  The numbers themselves are held to their references by tests/test_gpu_sh_support.py,
test_gpu_mldist.py, test_gpu_ancestral.py and test_gpu_parsimony.py, whose helpers these tests use."""
import numpy as np
import pytest

from gpu_common import synthetic_pair
from test_gpu_ancestral import SEED as ANC_SEED, SMALL_SHAPES, indices
from test_gpu_mldist import MDL, WANT, make_instance as dist_instance, synth_chars, synth_model
from test_gpu_sh_support import SEED, load, make_instance as sh_instance

pytestmark = pytest.mark.gpu


def same(a, b):
    """two answers of sh_support(..., want=("sums", "accepted")): SH, RELL, totals, sums and accepted flags bit for bit"""
    return a[:2] == b[:2] and np.array_equal(a[2], b[2]) and all(a[3][k].tobytes() == b[3][k].tobytes() for k in ("sums", "accepted"))


@pytest.mark.parametrize("kind", ["plain", "two_shards"])
def test_sh_support_work_space_regrows_with_the_table_on_the_device(kind):
    """8, then 4096, then 8 replicates on one instance: the second call frees and re-allocates the work space that held the uploaded
    alias table, the third finds it larger than it needs.  Each answer is a fresh instance's, called once with that count (replicate
    r is the same whatever the count, so the 8 are also the first 8 of the 4096)."""
    P = 70
    rng = np.random.default_rng(11)
    w = 1.0 + (np.arange(P) % 3)
    lks = -5.0 - 3.0 * rng.random((3, P))
    kw = dict(devices=[0, 0], force_sharded=True) if kind == "two_shards" else {}
    sites = int(w.sum())

    def answer(inst, reps):
        return inst.sh_support(sites, reps, SEED, want=("sums", "accepted"))

    f = sh_instance(P, w, **kw)
    try:
        load(f, lks)
        fresh_4096 = answer(f, 4096)
    finally:
        f.close()
    inst = sh_instance(P, w, **kw)
    try:
        assert kind == "plain" or len(inst.shard_ranges()) == 2
        load(inst, lks)
        fresh_8 = answer(inst, 8)            # (this instance IS a fresh one called once with 8)
        assert same(answer(inst, 4096), fresh_4096)
        assert same(answer(inst, 8), fresh_8)
        assert not np.array_equal(fresh_8[3]["sums"], fresh_4096[3]["sums"][-8:]) and fresh_8[3]["sums"].tobytes() == fresh_4096[3]["sums"][:8].tobytes()
    finally:
        inst.close()


@pytest.mark.parametrize("ns", [4, 20])
def test_pairwise_work_space_regrows(ns):
    """First without the counts, then with them (the work space gains a band of normalised counts): every array a fresh instance's"""
    mod = synth_model(ns)
    chars = synth_chars(5, 70, ns)
    w = 1.0 + (np.arange(70) % 3)
    f = dist_instance(chars, w, mod)
    try:
        D0, e0 = f.pairwise_ml_distances(MDL, want=WANT)
    finally:
        f.close()
    inst = dist_instance(chars, w, mod)
    try:
        assert inst.pairwise_ml_distances(MDL).tobytes() == D0.tobytes()
        D, e = inst.pairwise_ml_distances(MDL, want=WANT)
        assert D.tobytes() == D0.tobytes() and all(e[k].tobytes() == e0[k].tobytes() for k in WANT)
    finally:
        inst.close()


@pytest.mark.parametrize("ns", sorted(SMALL_SHAPES))
def test_node_posteriors_profile(ns):
    """Two profiled calls: two calls and a positive kernel time are read, once"""
    n, P = SMALL_SHAPES[ns]
    t, ot, tree, st = synthetic_pair(n, P, ns, 4, seed=ANC_SEED, ambiguous_every=5)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        sides, mats = indices(t, ot)
        t.inst.profile(1)
        a = t.inst.node_state_posteriors(sides, mats)
        b = t.inst.node_state_posteriors(sides, mats)
        ms, calls = t.inst.profile_read_node_posteriors()
        assert calls == 2 and ms > 0, (ms, calls)
        assert t.inst.profile_read_node_posteriors() == (0.0, 0)
        t.inst.profile(0)
        assert a.tobytes() == b.tobytes()
    finally:
        t.close()


def side_buffer_of(t, edge, node):
    """the buffer of `edge`'s side that holds `node` (a tip: its own index)"""
    e = t.edge(edge).contents
    if node == e.left.contents.num:
        return e.p_lk_left_idx
    return e.p_lk_tip_idx if e.rght.contents.tax else e.p_lk_rght_idx


def post_order_towards_tip_0(t):
    """(operations (dest, child1, child2) of the whole tree seen from tip 0, the two buffers of tip 0's edge)"""
    ops = []

    def walk(a, d, e):
        nd = t.node(d).contents
        if nd.tax:
            return
        kids = []
        for i in range(3):
            v = nd.v[i].contents.num
            if v != a:
                walk(d, v, nd.b[i].contents.num)
                kids.append(side_buffer_of(t, nd.b[i].contents.num, v))
        ops.append((side_buffer_of(t, e, d), kids[0], kids[1]))

    n0 = t.node(0).contents
    walk(0, n0.v[0].contents.num, n0.b[0].contents.num)
    return ops, (ops[-1][0], side_buffer_of(t, n0.b[0].contents.num, 0))


def test_parsimony_between_resident_served_evaluations():
    """A chain of dLk calls served by the resident workgroups, the parsimony calls, the chain again: the same doubles, every one of
    them served again, none launched instead -- the parsimony entry points are queries that keep the resident workgroups."""
    t, ot, tree, st = synthetic_pair(14, 382, 4, 4, seed=23, ambiguous_every=17)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        e = 3
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        chain = lambda: [t.dLk(0.003 * (i + 1), e)[1] for i in range(6)]
        first = chain()
        served, _, _, instead = t.inst.resident_stats(0)
        assert served > 0
        ops, (b1, b2) = post_order_towards_tip_0(t)
        assert len(ops) == 14 - 2
        t.inst.set_parsimony(False)
        t.inst.update_partial_parsimony(ops)
        score = t.inst.edge_parsimony(b1, b2)
        site = t.inst.site_parsimony()
        assert score == int(site.sum()) and score >= 3        # (unit weights; four states are all seen)
        t.inst.profile_read_parsimony()
        again = chain()
        assert first == again
        now = t.inst.resident_stats(0)
        assert now[0] == served + len(again) and now[3] == instead, (served, instead, now)
        t.Set_Use_Eigen_Lr(False)
    finally:
        t.close()
