"""The entry points that read partials or scale vectors from MEMORY with a kernel of their own, behind a ONE-SIDED whole-tree traversal
that left most of its results unstored (virtual, deferred, chained: phyml_amd/csrc/phyhip_unstored.hip): the regraft scan and the
mixture regraft scan (`regraft_make_real`, phyhip_scan.hpp), phyhip_optimise_triples (phyhip_triple.hip),
phyhip_calculate_node_state_posteriors (phyhip_ancestral.hip) and the tree-per-class MIXT_dLk (`mixture_dlnl_impl`,
phyhip_mixture.hip).  Each of them asks for its operands by name; an operand it forgot -- or one its own launch left unstored again
-- is allocated memory holding an older value, and the call returns a plausible number.

The state every case starts from (`Plan` on the CPU, `Case` / `MixtureCase` on the device): both sides at the tree's lengths A
(every buffer holds finite values), every edge at new lengths B, a one-sided Lk(NULL).  Memory under an unstored buffer then holds its
value at A, its definition says its value at B.  The twin `t0` stores every buffer; the oracle tree `ot` follows the same calls, and
its down-vectors at A are kept (`Plan.at_a`).  Targets come from `Replay` (tests/test_gpu_chained.py): (d, c) = a dependant and its
unstored input in the middle of a chain, and a virtual cherry.

Three moments: behind the LAUNCHED traversal (that state); behind a QUEUED one -- every edge at lengths C, Post_Order_Lk from the
root queued and not evaluated: the call stores the definitions at B in front of a list that writes the same buffers again; and the
same queue OVER STORED buffers -- every buffer of the traversal read back first, so that memory holds its value at B and nothing
stands in front: the call's own flush launches a list that would leave the named buffers unstored again, on that older value, and
only `Unstored::kept` keeps `defer_forwarded` and the virtual rule from it (in the second moment the definition in front makes a
second write of the buffer, which alone rules it out).

Held in every case: (1) every returned array and scalar equal to the all-stored twin's, bit for bit; (2) the unit's own CPU
reference on the all-stored vectors, at the unit's own bar (imported from its test); (3) that reference on the A-vectors in place of
c's and d's lies OUTSIDE that bar (CPU only: `test_stale_vectors_lie_outside_every_bar`, and again inside each device test); (4) the
on-demand counters rose by at least the unstored closure of the named buffers, and the instance's other state did not move; (5) the
dependant first, then every buffer of the traversal in reverse list order read back equal to the twin's copy, and the next Lk(NULL)
equal on both twins.

MIXT_dLk's kernel reads only the operands' scale vectors, which are zero at these tree depths; the stale value is planted
(phyhip_set_scale_factors on the stored buffer, then a traversal that rewrites it unstored), and what a stale read would return is
taken from the twin while the planted exponents stand there."""
import contextlib
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ancestral_ref as ar
import mixture_regraft_common as mrc
import triple_ref
from gpu_common import synthetic_oracle
from phyml_amd import capi
from test_gpu_ancestral import FLOOR, TOL, assert_close, indices
from test_gpu_chained import IDS, SHAPES, Replay, assert_reads_back, copies, edge_between, one_sided_keys, pair
from test_gpu_mixture_regraft import FIXTURE_OF, Mixture
from test_gpu_regraft import LEFT, Checker, within_bar
from test_gpu_triple import _bounds, _candidate, _staged

TRIPLE_SHAPES, TRIPLE_IDS = SHAPES[:-1], IDS[:-1]           # (phyhip_optimise_triples refuses groups)
# (states, patterns, taxa, seed) of the two mixture readers, K = 2 classes of one category: the chained tests' trees of 12 and 16 taxa
MIX_SHAPES, MIX_IDS = [(4, 300, 12, 1), (20, 90, 16, 6)], ["nt4_12x300", "lg4x_16x90"]
POSITIONS = ["child1", "child2", "subtree"]
MOMENTS = ["launched", "queued", "queued_over_stored"]
KEEP = 0                                                     # the kept record: the one that names c (as the subtree, in that position's case)


def lengths_b(e):
    return 0.02 + 0.01 * (e % 17)


def lengths_c(e):
    return 0.33 - 0.012 * (e % 23)


@pytest.fixture(autouse=True)
def _wall_time(request):
    t = time.perf_counter()
    yield
    print("wall time of", request.node.name, "%.2f s" % (time.perf_counter() - t))


# ---- the CPU half: the oracle tree in the start state, the targets, the stale vectors ---------------------------------------------
class Plan:
    """ot in the start state; rp: Replay; keys: the buffers of the one-sided traversal in list order; at_a: their vectors at A;
    c, d, above, cherry, stored, plain: node numbers (plain: an internal node whose three outer vectors are all stored)."""

    def __init__(self, ot):
        self.ot = ot
        ot.lk(None)
        self.rp = rp = Replay(ot)
        self.keys = one_sided_keys(ot, rp)
        ot.lk(None, both_sides=True)
        self.at_a = {k: (ot.plk[k].copy(), ot.scale[k].copy()) for k in self.keys}
        self.relen(lengths_b)
        ot.lk(None)
        self.at_b = {k: (ot.plk[k].copy(), ot.scale[k].copy()) for k in self.keys}
        self.memory = self.at_a                                                 # what memory holds under an unstored buffer
        self.site_lnl = ot.c_lnL_sorted.copy()
        assert rp.mid_chain(), "no buffer in the middle of a chain"
        self.d, self.c = rp.mid_chain()
        self.above = next(v for (v, be) in ot.adj[self.d] if be == rp.key[self.d][0])
        assert self.above >= ot.n and self.above in rp.key
        under_d = self.closure([self.d])
        self.cherry = sorted(rp.virt, key=lambda v: (v in under_d, v))[0]       # one outside d's closure where there is one
        self.stored = rp.order[-1]                                              # (read by the evaluation: always stored)
        assert not rp.unstored(self.stored)
        self.plain = next(x for x in rp.order if not any(v >= ot.n and rp.unstored(v) for v in self.children(x)))

    def relen(self, f):
        for e in range(self.ot.ne):
            self.ot.len[e] = f(e)
            self.ot.update_pmat(e)

    def queue(self, over_stored=False):
        """what the queued post-order from the root will have written; over_stored: every buffer was read back (stored at B) first"""
        if over_stored:
            self.memory = self.at_b
        self.relen(lengths_c)
        self.ot.post_order(self.ot.tip_root, self.ot.adj[self.ot.tip_root][0][0])

    def children(self, x):
        return [v for (v, be) in self.ot.adj[x] if be != self.rp.key[x][0]]

    def closure(self, nodes):
        """the unstored buffers whose definitions must be stored to make `nodes` real: the nodes' own, and transitively the unstored
        inputs of a deferred or chained one"""
        rp, seen, stack = self.rp, set(), [x for x in nodes if x >= self.ot.n and self.rp.unstored(x)]
        while stack:
            x = stack.pop()
            if x not in seen:
                seen.add(x)
                stack += [k for k in (rp.chained.get(x) or rp.deferred.get(x) or []) if k >= rp.n and rp.unstored(k)]
        return seen

    @contextlib.contextmanager
    def stale(self):
        """what memory holds (the A-vectors; over stored buffers the B-vectors) in place of c's and d's, in the oracle tree's own arrays"""
        ot, held = self.ot, {}
        for x in (self.c, self.d):
            k = self.rp.key[x]
            held[k] = (ot.plk[k].copy(), ot.scale[k].copy())
            ot.plk[k][...], ot.scale[k][...] = self.memory[k]
        try:
            yield
        finally:
            for k, (p, s) in held.items():
                ot.plk[k][...], ot.scale[k][...] = p, s

    @contextlib.contextmanager
    def preserved(self):
        """a CPU search writes the node's own vectors, the edge's products and lengths: put back afterwards"""
        ot = self.ot
        held = ({k: v.copy() for k, v in ot.plk.items()}, {k: v.copy() for k, v in ot.scale.items()}, ot.len.copy(), ot.pm.copy())
        try:
            yield
        finally:
            for k in ot.plk:
                ot.plk[k][...], ot.scale[k][...] = held[0][k], held[1][k]
            ot.len[...], ot.pm[...] = held[2], held[3]

    # -- reader 1 / 2: the records of one operand position
    def records(self, index_of, pos):
        """8 records: c, d and the cherry named in position `pos` ONLY (with and without LEFT), tips and a stored buffer everywhere
        else -- a position the call forgot to make real is then read from memory"""
        b = lambda x: index_of(self.rp.key[x])
        s, t1, t2 = b(self.stored), 1, 2
        recs = []
        for x in (self.c, self.d, self.cherry):
            recs += {"child1": [(b(x), s, t2, 0), (b(x), t1, s, LEFT)], "child2": [(t1, b(x), s, 0), (s, b(x), s, LEFT)],
                     "subtree": [(s, t1, b(x), 0), (t2, t1, b(x), LEFT)]}[pos]
        recs += [(t1, t2, s, 0), (s, t2, t1, 0)]
        ln = np.random.default_rng(5).uniform(0.01, 0.5, (len(recs), 3))
        return [r + tuple(float(v) for v in l) for r, l in zip(recs, ln)]

    def scan_named(self):
        return [self.c, self.d, self.cherry]

    # -- reader 3 / 4: the nodes
    def triple_nodes(self):
        return [self.d, self.above]

    def posterior_nodes(self):
        return [self.plain, self.d, self.above]      # (a call that stores the first 2n of its 3n sides misses the last node's)

    def node_named(self, nodes):
        """the down-buffers among the outer vectors of `nodes`"""
        return [v for x in nodes for v in self.children(x) if v >= self.ot.n]

    def first_search(self, a):
        """(lkBegin, B_lnl) of the first search of Triple_Dist at node a from the tree's lengths: it reads all three outer vectors"""
        with self.preserved():
            e = triple_ref.edges_of(self.ot, a)
            self.ot.update_partial(e[0], a)
            s = triple_ref.br_len_opt(self.ot, e[0])
            return s.lk_begin, _bounds(self.ot, s.result)[0]

    def posteriors(self, nodes):
        return ar.node_posteriors(self.ot, nodes, site_lnl=self.site_lnl)[0]

    # -- item 3: the same references on the A-vectors lie outside the bar
    def assert_scan_tells_stale_from_fresh(self, candidate, cands, what):
        """candidate(record) -> lnL on the oracle tree's vectors as they stand"""
        fresh = [candidate(r) for r in cands[:4]]                 # (the records of c and d)
        with self.stale():
            old = [candidate(r) for r in cands[:4]]
        for r, u, v in zip(cands[:4], old, fresh):
            assert not within_bar(u, v), (what, "a stale operand is not told from a fresh one", r, u, v)

    def assert_nodes_tell_stale_from_fresh(self, what):
        fresh = {a: self.first_search(a) for a in self.triple_nodes()}
        post = self.posteriors(self.posterior_nodes())
        with self.stale():
            old = {a: self.first_search(a) for a in self.triple_nodes()}
            post_old = self.posteriors(self.posterior_nodes())
        for a in self.triple_nodes():
            assert abs(old[a][0] - fresh[a][0]) > old[a][1] + fresh[a][1], (what, "Triple_Dist", a, old[a], fresh[a])
        differs = np.abs(post_old - post) > TOL * np.maximum(np.abs(post), FLOOR)
        assert not differs[0].any() and differs[1].any() and differs[2].any(), (what, "posteriors", differs.sum(axis=(1, 2)))


def fake_index(ot):
    """buffer numbers for a CPU-only checker: any one-to-one numbering above the tips"""
    return lambda key: ot.n + 2 * key[0] + key[1]


def cpu_checker(ot, index_of):
    return Checker(ot, {index_of(k): (ot.plk[k], ot.scale[k]) for k in ot.plk})


def mixture_oracles(ns, P, n, seed, K=2):
    """the oracle half of Mixture.synthetic: (class oracle trees, factors, sums)"""
    d, models, factors, sums = mrc.fixture(FIXTURE_OF[ns])
    ot0, tree, st, tv, wg = synthetic_oracle(n, P, ns, 1, seed, 0.02, 0.3, None, 1, 5)
    ots = mrc.class_oracles(models[:K], n, tree.edge_left, tree.edge_rght, tree.edge_len, wg, ot0.tip_vec, ot0.tip_ds, ot0.tip_amb)
    return ots, factors[:K], sums


def mixture_checkers(plans, index_of):
    return [mrc.ClassChecker(p.ot, {index_of(k): (p.ot.plk[k], p.ot.scale[k]) for k in p.ot.plk}) for p in plans]


@contextlib.contextmanager
def all_stale(plans):
    with contextlib.ExitStack() as es:
        for p in plans:
            es.enter_context(p.stale())
        yield


def assert_mixture_scan_tells_stale_from_fresh(plans, factors, sums, chks, cands, what):
    ref = lambda r: mrc.mixture_candidate(chks, factors, sums, r)[0]
    fresh = [ref(r) for r in cands[:4]]
    with all_stale(plans):
        old = [ref(r) for r in cands[:4]]
    for r, u, v in zip(cands[:4], old, fresh):
        assert not mrc.within_bar(u, v), (what, "a stale operand is not told from a fresh one", r, u, v)


# ---- CPU only: the chosen trees give the targets, and every reference tells a stale operand from a fresh one ----------------------------
def test_the_chosen_trees_give_the_targets():
    for shape, name in list(zip(SHAPES, IDS)) + [((ns, 1, 8, n, seed, None), name) for (ns, P, n, seed), name in zip(MIX_SHAPES, MIX_IDS)]:
        ns, Cc, P, n, seed, _ = shape
        p = Plan(synthetic_oracle(n, 8, ns, Cc, seed, ambiguous_every=13)[0])
        rp = p.rp
        assert p.c in rp.chained or p.c in rp.deferred, name
        assert p.d in rp.chained and p.c in rp.chained[p.d] and p.cherry in rp.virt, name
        assert len(p.closure([p.d])) >= 2 and p.closure(p.node_named([p.above])) >= p.closure([p.d]), name      # a closure at least two deep
        assert p.d in p.children(p.above) and p.c in p.children(p.d), name
        assert p.node_named([p.plain]) == [] or not any(rp.unstored(v) for v in p.node_named([p.plain])), name
        for pos in POSITIONS:   # each target in that position only, with and without LEFT
            recs = p.records(fake_index(p.ot), pos)
            at = POSITIONS.index(pos)
            for x in p.scan_named():
                b = fake_index(p.ot)(rp.key[x])
                mine = [r for r in recs if b in r[:3]]
                assert len(mine) == 2 and {r[3] for r in mine} == {0, LEFT} and all(r[at] == b and r[:3].count(b) == 1 for r in mine), (name, pos)
            assert 8 <= len(recs) <= 12 and fake_index(p.ot)(rp.key[p.c]) in recs[KEEP][:3]


@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stale_vectors_lie_outside_every_bar(shape, moment):
    """item (3) for the scan, Triple_Dist and the posteriors, at the shapes and lengths the device tests use"""
    ns, Cc, P, n, seed, _ = shape
    p = Plan(synthetic_oracle(n, P, ns, Cc, seed, ambiguous_every=13)[0])
    if moment != "launched":
        p.queue(moment == "queued_over_stored")
    index_of = fake_index(p.ot)
    chk = cpu_checker(p.ot, index_of)
    for pos in POSITIONS:
        p.assert_scan_tells_stale_from_fresh(lambda r: chk.candidate(r)[0], p.records(index_of, pos), (IDS[SHAPES.index(shape)], moment, pos))
    assert P <= capi.TRIPLE_MAX_PATTERNS
    p.assert_nodes_tell_stale_from_fresh((IDS[SHAPES.index(shape)], moment))


@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", MIX_SHAPES, ids=MIX_IDS)
def test_stale_vectors_lie_outside_the_mixture_bar(shape, moment):
    ns, P, n, seed = shape
    ots, factors, sums = mixture_oracles(ns, P, n, seed)
    plans = [Plan(ot) for ot in ots]
    if moment != "launched":
        for p in plans:
            p.queue(moment == "queued_over_stored")
    assert len({(p.c, p.d, p.cherry) for p in plans}) == 1          # (one topology: the same targets in every class)
    index_of = fake_index(ots[0])
    chks = mixture_checkers(plans, index_of)
    for pos in POSITIONS:
        assert_mixture_scan_tells_stale_from_fresh(plans, factors, sums, chks, plans[0].records(index_of, pos), (shape, moment, pos))


# ---- the device half -------------------------------------------------------------------------------------------------------------
def unstored_now(inst):
    return inst.virtual_stats()[0] + inst.deferred_stats()[0] + inst.chained_stats()[0]


def on_demand(inst):
    return inst.virtual_stats()[3] + inst.deferred_stats()[2] + inst.chained_stats()[2]


def other_state(t):
    return (t.inst.site_outputs(), t.inst.get_dot_prod(), t.inst.numerical_warning(), [t.inst.get_transition_matrix(k) for k in range(t.ne + 4)])


def assert_same_state(before, after, what):
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])), (what, "site outputs")
    assert np.array_equal(before[1], after[1]) and before[2] == after[2], (what, "eigen products / warning")
    assert all(np.array_equal(a, b) for a, b in zip(before[3], after[3])), (what, "matrices")


def relen(trees, f):
    for x in trees:
        for e in range(x.ne):
            x.edge(e).contents.l = f(e)
            x.Update_PMat_At_Given_Edge(e)


def to_start_state(t, t0, plan):
    """steps 1-5 on the twins (the oracle tree has taken them: Plan); returns how many buffers of t are unstored"""
    for x in (t, t0):
        x.Set_Both_Sides(True)
    assert t.Lk(None) == t0.Lk(None)
    relen((t, t0), lengths_b)
    for x in (t, t0):
        x.Set_Both_Sides(False)
    assert t.Lk(None) == t0.Lk(None)
    assert t.inst.chained_stats()[0] == len(plan.rp.chained)
    assert unstored_now(t0.inst) == 0
    return unstored_now(t.inst)   # (the chained ones, and the deferred and virtual ones of both traversals)


def store_all(t, plan):
    """every buffer of the traversal read back in list order: stored, at its value at B"""
    for k in plan.keys:
        t.partials(*k)
    assert t.inst.chained_stats()[0] == 0


def queue_traversal(trees):
    """every edge at lengths C, the post-order from the root queued and not evaluated"""
    relen(trees, lengths_c)
    for x in trees:
        x.Post_Order_Lk(0, x.node(0).contents.v[0].contents.num)


class Case:
    """The twins in the start state at one of the two moments, and what is held around every reader's call"""

    def __init__(self, shape, moment):
        self.t, self.t0, ot = pair(shape)
        try:
            self.plan = Plan(ot)
            self.moment = moment
            self.unstored = to_start_state(self.t, self.t0, self.plan)
            if moment == "queued_over_stored":
                store_all(self.t, self.plan)
            if moment != "launched":
                relen((self.t, self.t0), lengths_c)
            self.before_state = other_state(self.t)
            if moment != "launched":
                queue_traversal((self.t, self.t0))
                self.plan.queue(moment == "queued_over_stored")
            self.mark = on_demand(self.t.inst)
        except Exception:
            self.close()
            raise

    def close(self):
        self.t.close(); self.t0.close()

    def buf(self, x):
        return self.t.side_buffer(*self.plan.rp.key[x])

    def on_both(self, call):
        """the call on the all-stored twin (whose copies of the traversal's buffers are taken first) and on t"""
        self.want = copies(self.t0, self.plan.keys)
        ref = call(self.t0)
        return call(self.t), ref

    def afterwards(self, named, what):
        """items (4) and (5)"""
        t, t0, p = self.t, self.t0, self.plan
        need = p.closure(named)
        if self.moment != "queued_over_stored":
            assert need and on_demand(t.inst) - self.mark >= len(need), (what, on_demand(t.inst) - self.mark, sorted(need))
        if self.moment != "launched":   # the call's own launch left what it named stored; the rest may be unstored again
            assert unstored_now(t.inst) <= self.unstored - len([x for x in set(named) if p.rp.unstored(x)]), (what, unstored_now(t.inst), self.unstored)
        assert_same_state(self.before_state, other_state(t), what)
        assert_reads_back(t, p.rp.key[p.d], self.want[p.rp.key[p.d]])
        for k in p.keys[::-1]:
            assert_reads_back(t, k, self.want[k])
        assert t.Lk(None) == t0.Lk(None)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_regraft_scan(shape, moment, pos):
    cs = Case(shape, moment)
    try:
        p, t = cs.plan, cs.t
        what = ("regraft scan", moment, pos)
        cands = p.records(lambda k: t.side_buffer(*k), pos)
        assert cs.buf(p.c) in cands[KEEP][:3]

        def call(x):
            lnl, warn = x.inst.regraft_log_likelihoods(cands, keep=KEEP, with_warnings=True)
            return (lnl, warn) + x.inst.regraft_partials()
        got, ref = cs.on_both(call)
        for u, v in zip(got, ref):
            assert np.array_equal(u, v), (what, "against the all-stored twin", u, v)
        chk = Checker.of_tree(t, p.ot)
        w = p.ot.wght > 0
        for k, r in enumerate(cands):
            lnl, warn, vec, sc, _ = chk.candidate(r)
            assert within_bar(got[0][k], lnl) and got[1][k] == warn, (what, k, r, got[0][k], lnl)
            if k == KEEP:
                assert np.array_equal(got[2][w], vec[w]) and np.array_equal(got[3][w], sc[w]), (what, "kept vector")
        p.assert_scan_tells_stale_from_fresh(lambda r: chk.candidate(r)[0], cands, what)
        cs.afterwards(p.scan_named(), what)
    finally:
        cs.close()


@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", TRIPLE_SHAPES, ids=TRIPLE_IDS)
def test_triple_dist_scan(shape, moment):
    cs = Case(shape, moment)
    try:
        p, t = cs.plan, cs.t
        what = ("Triple_Dist", moment)
        nodes = p.triple_nodes()
        cands = [_candidate(t, a) for a in nodes]
        assert cands == [_candidate(cs.t0, a) for a in nodes]
        assert cs.buf(p.c) in cands[0][0] and cs.buf(p.d) in cands[1][0]
        res, ref = cs.on_both(lambda x: x.inst.optimise_triples(cands))
        got, ref = [r.as_tuple() for r in res], [r.as_tuple() for r in ref]
        assert got == ref, (what, "against the all-stored twin", got, ref)
        for a, c, r in zip(nodes, cands, res):
            with p.preserved():
                _staged(p.ot, a, c, r, what)
        p.assert_nodes_tell_stale_from_fresh(what)
        cs.afterwards(p.node_named(nodes), what)
    finally:
        cs.close()


@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_node_state_posteriors(shape, moment):
    cs = Case(shape, moment)
    try:
        p, t = cs.plan, cs.t
        what = ("posteriors", moment)
        nodes = p.posterior_nodes()
        sides, mats = indices(t, p.ot, nodes)
        assert cs.buf(p.c) in sides[1] and cs.buf(p.d) in sides[2] and cs.buf(p.d) not in sides[:2]
        got, ref = cs.on_both(lambda x: x.inst.node_state_posteriors(sides, mats, p.site_lnl, with_warning=True))
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (what, "against the all-stored twin")
        assert_close(got[0], p.posteriors(nodes), what)
        p.assert_nodes_tell_stale_from_fresh(what)
        cs.afterwards(p.node_named(nodes), what)
    finally:
        cs.close()


# ---- the two mixture readers ------------------------------------------------------------------------------------------------------
class MixtureCase:
    """Case for the class trees of a mixture: M (thresholds 3 / 3 on every class tree) and the all-stored M0, one Plan per class"""

    def __init__(self, shape, moment, queue_now=True):
        ns, P, n, seed = shape
        self.M = self.M0 = None
        try:
            self.M = Mixture.synthetic(ns, P, K=2, n=n, seed=seed, evaluate=False)
            self.M0 = Mixture.synthetic(ns, P, K=2, n=n, seed=seed, evaluate=False)
            self.plans = [Plan(ot) for ot in self.M.ots]
            self.moment, self.unstored = moment, []
            for t, t0, p in zip(self.M.trees, self.M0.trees, self.plans):
                t.inst.set_virtual_buffers(3)
                t.inst.set_chained_buffers(3)
                t0.inst.set_virtual_buffers(0)
                self.unstored.append(to_start_state(t, t0, p))
            if queue_now:
                self.at_the_moment()
        except Exception:
            self.close()
            raise

    def at_the_moment(self, store=True):
        both = self.M.trees + self.M0.trees
        if self.moment == "queued_over_stored" and store:
            for t, p in zip(self.M.trees, self.plans):
                store_all(t, p)
        if self.moment != "launched":
            relen(both, lengths_c)
        self.before_state = [other_state(t) for t in self.M.trees]
        if self.moment != "launched":
            queue_traversal(both)
            for p in self.plans:
                p.queue(self.moment == "queued_over_stored")
        self.mark = [on_demand(t.inst) for t in self.M.trees]

    def close(self):
        for m in (self.M, self.M0):
            if m is not None:
                m.close()

    def on_both(self, call):
        self.want = [copies(t0, p.keys) for t0, p in zip(self.M0.trees, self.plans)]
        ref = call(self.M0)
        return call(self.M), ref

    def afterwards(self, named, what, state=True):
        for k, (t, t0, p) in enumerate(zip(self.M.trees, self.M0.trees, self.plans)):   # every class instance
            need = p.closure(named)
            if self.moment != "queued_over_stored":
                assert need and on_demand(t.inst) - self.mark[k] >= len(need), (what, k, on_demand(t.inst) - self.mark[k], sorted(need))
            if self.moment != "launched":
                assert unstored_now(t.inst) <= self.unstored[k] - len([x for x in set(named) if p.rp.unstored(x)]), (what, k)
            if state:
                assert_same_state(self.before_state[k], other_state(t), (what, k))
            assert_reads_back(t, p.rp.key[p.d], self.want[k][p.rp.key[p.d]])
            for key in p.keys[::-1]:
                assert_reads_back(t, key, self.want[k][key])
            assert t.Lk(None) == t0.Lk(None)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", MIX_SHAPES, ids=MIX_IDS)
def test_mixture_regraft_scan(shape, moment, pos):
    cs = MixtureCase(shape, moment)
    try:
        M, p = cs.M, cs.plans[0]
        what = ("mixture regraft scan", moment, pos)
        assert all(t.side_buffer(*k) == M.trees[0].side_buffer(*k) for t in M.trees + cs.M0.trees for k in p.ot.plk)
        cands = p.records(lambda k: M.trees[0].side_buffer(*k), pos)

        def call(m):
            lnl, warn = m.scan(cands, keep=KEEP, with_warnings=True)
            return [lnl, warn] + [v for cl in range(m.K) for v in m.first.mixture_regraft_partials(cl)]
        got, ref = cs.on_both(call)
        for u, v in zip(got, ref):
            assert np.array_equal(u, v), (what, "against the all-stored twin", u, v)
        chks = M.checkers()
        w = p.ot.wght > 0
        for k, r in enumerate(cands):
            lnl, warn, per = M.reference(chks, r)
            assert mrc.within_bar(got[0][k], lnl) and got[1][k] == warn, (what, k, r, got[0][k], lnl)
            if k == KEEP:
                for cl in range(M.K):
                    assert np.array_equal(got[2 + 2 * cl][w], per[cl][2][w]) and np.array_equal(got[3 + 2 * cl][w], per[cl][3][w]), (what, "kept vector", cl)
        assert_mixture_scan_tells_stale_from_fresh(cs.plans, M.factors, M.sums, chks, cands, what)
        cs.afterwards(p.scan_named(), what)
    finally:
        cs.close()


@pytest.mark.parametrize("unstored_operand", ["left", "right"])
@pytest.mark.parametrize("moment", MOMENTS)
@pytest.mark.parametrize("shape", MIX_SHAPES, ids=MIX_IDS)
def test_tree_per_class_mixt_dlk(shape, moment, unstored_operand):
    """Update_Eigen_Lr in every class at the edge (d, c); exponents planted in c's stored scale vector; then the traversal that
    rewrites c and leaves it unstored: memory under c holds the planted exponents, its definition the computed ones -- and, at the
    queued moment, the traversal queued again at lengths C behind that; over stored buffers that second traversal is left out, and
    the queued one rewrites the stored c.  c's buffer is passed as the left or as the right operand (the kernel adds the two vectors)."""
    cs = MixtureCase(shape, moment, queue_now=False)
    try:
        M, M0, p = cs.M, cs.M0, cs.plans[0]
        what = ("MIXT_dLk", moment, unstored_operand)
        e_c = edge_between(p.ot, p.d, p.c)
        k_c = p.rp.key[p.c]
        assert k_c[0] == e_c and p.rp.unstored(p.c)
        mine, other = M.trees[0].side_buffer(*k_c), M.trees[0].side_buffer(e_c, 1 - k_c[1])
        lefts, rights = ([mine] * M.K, [other] * M.K) if unstored_operand == "left" else ([other] * M.K, [mine] * M.K)
        call = lambda m: capi.mixture_eigen_lnl_dlnl(m.ids, lefts, rights, 0.07, *m.coef())
        for m in (M, M0):
            for cl, t in enumerate(m.trees):
                t.Set_Update_Eigen_Lr(True); t.Update_Eigen_Lr(e_c); t.Set_Update_Eigen_Lr(False)
                planted = np.zeros(p.ot.P, np.int32)
                planted[10:20] = 2 + 3 * cl
                capi._chk(t.inst.L.phyhip_set_scale_factors(t.inst.id, mine, capi._ptr(planted)))
        stale, stale0 = call(M), call(M0)          # what a read of the planted exponents returns
        assert stale == stale0
        if moment != "queued_over_stored":         # the second one-sided traversal: the operands are unstored again
            for t, t0 in zip(M.trees, M0.trees):
                assert t.Lk(None) == t0.Lk(None)
                assert t.inst.chained_stats()[0] == len(p.rp.chained) and (p.c in p.rp.chained or t.inst.deferred_stats()[0] >= len(p.rp.deferred))   # c among them
        cs.at_the_moment(store=False)              # (over stored buffers: c stands in memory with the planted exponents)
        got, ref = cs.on_both(call)
        assert got == ref, (what, "against the all-stored twin", got, ref)
        # (3) the planted exponents move lnL and dlnL far beyond any rounding of the sums
        print(what, "on the planted exponents", stale0, "on the computed ones", ref)
        assert abs(ref[1] - stale0[1]) > 1e-6 * abs(ref[1]), (what, ref, stale0)
        cs.afterwards([p.c], what, state=False)    # (Update_Eigen_Lr has written the eigen products since the state was taken)
    finally:
        cs.close()


# ---- one stream ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,C,P,devices", [(4, 4, 300, None), (20, 4, 90, None), (4, 4, 700, (0, 0))])
def test_random_call_streams_with_side_calls(ns, C, P, devices):
    """tests/test_gpu_chained.py's stream (the same actions and threshold moves) with four more actions: a regraft scan of 6 random
    records, posteriors at 3 random internal nodes, phyhip_optimise_triples at 2 random nodes (not on the sharded pair) and the exact
    per-site route at a random edge.  Every answer equal to the run that stores every buffer; every buffer read back at the end."""
    from gpu_common import synthetic_pair
    dev = None if devices is None else list(devices)
    t, ot, tree, st = synthetic_pair(34, P, ns, C, seed=21, host_pmat=True, ambiguous_every=13, devices=dev)
    t0, _, _, _ = synthetic_pair(34, P, ns, C, seed=21, host_pmat=True, ambiguous_every=13, devices=dev)
    try:
        t0.inst.set_virtual_buffers(0)
        t.inst.set_chained_buffers(3)
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)   # (every buffer written once)
        rng = np.random.default_rng(int(os.environ.get("PHYHIP_FUZZ_SEED", "23")))
        internal = [e for e in range(t.ne) if ot.el[e] >= ot.n and ot.er[e] >= ot.n]
        keys = list(ot.plk)
        buffers = [t.side_buffer(*k) for k in keys]
        nodes = ar.internal_nodes(ot)
        site_lnl = np.full(P, -40.0)
        n_act = 15 if devices is None else 14
        chained_seen, ran = 0, {11: 0, 12: 0, 13: 0, 14: 0}
        for it in range(int(os.environ.get("PHYHIP_FUZZ_ITERS", "150"))):
            act = int(rng.integers(0, n_act))
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
            elif act == 9:
                if it % 4 == 0:
                    t.inst.set_virtual_buffers(int(rng.choice([0, 2, 16, 40])))   # (the thresholds move; 0 stores what is unstored)
                    t.inst.set_chained_buffers(int(rng.choice([0, 3, 3, 16])))
                else:
                    tip, pat = int(rng.integers(0, ot.n)), int(rng.integers(0, P))
                    v = np.zeros(ns); v[int(rng.integers(0, ns))] = 1.0
                    if rng.integers(0, 2):
                        v[:] = 1.0
                    for x in (t, t0):
                        x.inst.set_tip_partials_at_pattern(tip, pat, v)
            elif act == 11:   # a regraft scan over written buffers and tips
                pick = lambda: int(rng.integers(0, ot.n)) if rng.integers(0, 3) == 0 else int(rng.choice(buffers))
                cands = []
                for _ in range(6):
                    c1, c2, sub = pick(), pick(), pick()
                    flags = LEFT if sub >= ot.n and rng.integers(0, 2) else 0
                    cands.append((c1, c2, sub, flags) + tuple(float(v) for v in rng.uniform(0.005, 0.5, 3)))
                keep = int(rng.integers(0, 6))
                got, ref = [], []
                for x, out in ((t, got), (t0, ref)):
                    out.extend(x.inst.regraft_log_likelihoods(cands, keep=keep, with_warnings=True))
                    out.extend(x.inst.regraft_partials())
                assert all(np.array_equal(u, v) for u, v in zip(got, ref)), (it, cands)
            elif act == 12:   # posteriors
                pick = [int(a) for a in rng.choice(nodes, size=3, replace=False)]
                sides, mats = indices(t, ot, pick)
                got, ref = (x.inst.node_state_posteriors(sides, mats, site_lnl, with_warning=True) for x in (t, t0))
                assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (it, pick)
            elif act == 13:   # the exact per-site route
                e = int(rng.integers(0, t.ne))
                got, ref = t.Exact_Site_Lk(e), t0.Exact_Site_Lk(e)
                assert all(np.array_equal(u, v) for u, v in zip(got, ref)), (it, e)
            else:             # Triple_Dist at two nodes
                pick = [int(a) for a in rng.choice(nodes, size=2, replace=False)]
                cands = [_candidate(t, a) for a in pick]
                assert cands == [_candidate(t0, a) for a in pick]
                got, ref = ([r.as_tuple() for r in x.inst.optimise_triples(cands)] for x in (t, t0))
                assert got == ref, (it, pick)
            if act in ran:
                ran[act] += 1
        assert chained_seen > 0
        assert all(v > 0 for a, v in ran.items() if a < n_act), ran
        for x in (t, t0):
            x.Set_Both_Sides(True)
        assert t.Lk(None) == t0.Lk(None)
        for k in ot.plk:
            assert np.array_equal(t.partials(*k), t0.partials(*k)), k
            assert np.array_equal(t.scale_factors(*k), t0.scale_factors(*k)), k
    finally:
        t.close(); t0.close()
