"""phyhip_calculate_regraft_parsimony (phyml_amd/csrc/phyhip_pars.hip; Pars_Regraft_Scan in the host layer): K regraft candidates of
the parsimony SPR search in one device call.  Expected values come from the reference's own recorded candidates
(tests/golden/regraft_pars_<case>.npz) and from tests/pars_ref.py, which tests/test_pars_regraft_restatement.py holds to them --
never from the device's own per-candidate route; the host-layer test (10) is the one exception, and it checks index resolution only.
Everything is integer: every comparison is == / np.array_equal.  All through the C ABI."""
import numpy as np
import pytest

import pars_ref
import pars_regraft_ref as rr
from test_gpu_parsimony import lk_tree, make_instance, random_index, random_masks, random_step

pytestmark = pytest.mark.gpu


def _code(fn, *args, **kw):
    from phyml_amd import capi
    with pytest.raises(capi.PhyhipError) as ei:
        fn(*args, **kw)
    return ei.value.code


def kept(inst, general):
    """(J, site[]) of the kept candidate, J in pars_ref.Planes' form"""
    if general:
        return inst.regraft_partial_parsimony(general=True), inst.regraft_site_parsimony()
    return inst.regraft_partial_parsimony(), inst.regraft_site_parsimony()


def same_vector(got, want, general):
    return np.array_equal(got, want) if general else (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


class Pool:
    """a 7-taxon random tree with all its vectors on the device and in a pars_ref.Planes, and reference results of candidates,
    each computed once"""

    def __init__(self, P, ns, general, seed, wght=None, n=7, **kw):
        self.T = random_index(n, seed)
        self.n, self.P, self.ns, self.general = n, P, ns, general
        self.masks = random_masks(n, P, ns, seed + 1)
        self.w = np.random.RandomState(seed + 2).randint(0, 6, size=P).astype(np.float64) if wght is None else wght
        self.step = random_step(ns, seed + 3) if general else None
        self.ops = self.T.both_sides()
        self.spare = self.T.nbuf
        self.pl = pars_ref.Planes(self.masks, ns, self.step).run(self.ops)
        self.inst = make_instance(self.masks, ns, self.T.nbuf + 1, self.w, **kw)
        self.inst.set_parsimony(general, self.step)
        self.inst.update_partial_parsimony(self.ops)
        self.ref = {}

    def want(self, cand):
        """(sum, J, site[]) from pars_ref"""
        cand = tuple(int(x) for x in cand)
        if cand not in self.ref:
            J, site = rr.join_and_score(self.pl, self.spare, cand)
            J = J.copy() if self.general else (J[0].copy(), J[1].copy())
            self.ref[cand] = (pars_ref.weighted_sum(site, self.w), J, site.copy())
        return self.ref[cand]

    def check(self, cands, keep=-1, what=None):
        got = self.inst.regraft_parsimony(cands, keep=keep)
        assert got.dtype == np.int64 and len(got) == len(cands)
        for k, c in enumerate(cands):
            assert int(got[k]) == self.want(c)[0], (what, k, c, int(got[k]), self.want(c)[0])
        if keep >= 0:
            J, site = kept(self.inst, self.general)
            assert same_vector(J, self.want(cands[keep])[1], self.general), (what, keep)
            assert np.array_equal(site, self.want(cands[keep])[2]), (what, keep)
        return got

    def triples(self, count, seed, subtrees=3):
        """`count` distinct candidates over tips and inner vectors, few distinct subtrees"""
        rng = np.random.RandomState(seed)
        subs = rng.choice(self.T.nbuf, size=subtrees, replace=False)
        out = {(int(rng.randint(self.T.nbuf)), int(rng.randint(self.T.nbuf)), int(subs[rng.randint(subtrees)])) for _ in range(3 * count)}
        return sorted(out)[:count]

    def close(self):
        self.inst.close()


# ---- 1. the reference's recorded candidates ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("case", rr.CASES)
def test_fixtures(case, general):
    base, rg = rr.load(case)
    ns, sites = int(base["ns"][0]), rr.sites(case)
    c_key, s_key = ("c_pars_general", "site_general") if general else ("c_pars_fitch", "site_fitch")
    inst = make_instance(pars_ref.char_masks(base["seq"], ns), ns, max(s.nbuf for s in sites), base["wght"].astype(np.float64))
    try:
        inst.set_parsimony(general, base["step_mat"] if general else None)
        for s in sites:
            inst.update_partial_parsimony(s.ops)                 # the pruned topology's vectors: queued, not launched
            got = inst.regraft_parsimony(s.cands)                # every target of the site in one call
            assert [int(x) for x in got] == [int(rg[c_key][r]) for r in s.rows], (case, s.edge, s.link)
            if s_key not in rg:
                continue
            pl = rr.planes(base, general).run(s.ops)
            for k, (r, cand) in enumerate(zip(s.rows, s.cands)):  # each candidate kept in turn
                again = inst.regraft_parsimony(s.cands, keep=k)
                assert np.array_equal(again, got)
                J, site = kept(inst, general)
                assert np.array_equal(site, rg[s_key][r]), (case, s.edge, s.link, k)
                assert same_vector(J, rr.join_and_score(pl, s.spare, cand)[0], general), (case, s.edge, s.link, k)
    finally:
        inst.close()


# ---- 2. ragged shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("ns", [4, 20])
def test_ragged_shapes(ns, general):
    """pattern counts around the tile, and list lengths around the points at which the slabs of a launch grow by a record: with
    `want` slabs wanted, lists of up to `want` candidates have slabs of one record, want + 1 the first slabs of two, 2 want + 1 of
    three"""
    from phyml_amd import capi
    for P in (1, 2, 255, 256, 257, 513):
        pool = Pool(P, ns, general, 100 + P + ns)
        try:
            cu = pool.inst.details.computeUnits
            want = capi.pars_regraft_slabs(capi.PARS_REGRAFT_CHUNK, P, cu)[0]
            assert capi.pars_regraft_slabs(want, P, cu) == (want, 1) and capi.pars_regraft_slabs(want + 1, P, cu)[1] == 2
            tri = pool.triples(24, P)
            rng = np.random.RandomState(P)
            for K in (1, 2, want - 1, want, want + 1, 2 * want - 1, 2 * want, 2 * want + 1):
                # runs of one subtree and changes of it, wherever the slab boundaries fall
                cands = [tri[i] for i in np.sort(rng.randint(len(tri), size=K))] if K % 2 else [tri[i] for i in rng.randint(len(tri), size=K)]
                pool.check(cands, keep=K - 1 if K % 3 else K // 2, what=(ns, general, P, K))
        finally:
            pool.close()


# ---- 3. operand forms ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("ns", [4, 20])
def test_operand_forms(ns, general):
    from phyml_amd import capi
    P = 513
    pool = Pool(P, ns, general, 7 + ns)
    try:
        n, inner = pool.n, list(range(pool.n, pool.T.nbuf))
        a, b, c, d = inner[0], inner[1], inner[2], inner[-1]
        forms = {"tip as child1": (0, a, b), "tip as child2": (a, 1, b), "tip as subtree": (a, b, 2), "all three tips": (3, 4, 5),
                 "child1 == child2": (c, c, d), "child1 == child2, a tip": (6, 6, a), "all three the same vector": (d, d, d),
                 "subtree one of the children": (a, b, a)}
        for what, cand in forms.items():
            pool.check([cand], keep=0, what=what)
        pool.check(list(forms.values()), keep=3, what="all forms in one list")
        # lists long enough for slabs of several records: the subtree changes at every record, never, exactly at a slab boundary,
        # and one record to either side of it
        cu = pool.inst.details.computeUnits
        want = capi.pars_regraft_slabs(capi.PARS_REGRAFT_CHUNK, P, cu)[0]
        K = 3 * want
        slabs, size = capi.pars_regraft_slabs(K, P, cu)
        assert size == 3 and slabs == want
        kids = [(0, a), (b, 1), (c, d), (a, b), (5, 6), (d, d)]
        subs = [a, 2, d, b]
        lists = {"every record": [kids[k % 6] + (subs[k % 4],) for k in range(K)],
                 "never": [kids[k % 6] + (c,) for k in range(K)],
                 "at a slab boundary": [kids[k % 6] + (subs[(k // size) % 4],) for k in range(K)],
                 "one record behind a slab boundary": [kids[k % 6] + (subs[((k + size - 1) // size) % 4],) for k in range(K)],
                 "one record before a slab boundary": [kids[k % 6] + (subs[((k + 1) // size) % 4],) for k in range(K)]}
        for what, cands in lists.items():
            pool.check(cands, keep=size, what=what)
    finally:
        pool.close()


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general,ns", [(False, 4), (False, 20), (True, 4), (True, 20)])
def test_a_result_depends_on_the_candidate_alone(general, ns):
    pool = Pool(300, ns, general, 50 + ns)
    try:
        tri = pool.triples(30, 5)
        probe, rng = tri[0], np.random.RandomState(1)
        seen = []
        for K in (1, 64, 700):
            for place in sorted({0, K // 2, K - 1}):
                cands = [tri[1 + rng.randint(len(tri) - 1)] for _ in range(K)]
                cands[place] = probe
                got = pool.check(cands, keep=place, what=(K, place))
                J, site = kept(pool.inst, general)
                seen.append((int(got[place]), J, site))
        for s in seen[1:]:
            assert s[0] == seen[0][0] and same_vector(s[1], seen[0][1], general) and np.array_equal(s[2], seen[0][2])
    finally:
        pool.close()


# ---- 5. weights ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
def test_weights(general):
    from phyml_amd import capi
    P, ns = 257, 4
    pool = Pool(P, ns, general, 21)
    try:
        tri = pool.triples(12, 3)
        pool.check(tri, keep=1, what="small weights")
        for what, w in (("zeros", np.zeros(P)), ("up to 2^40", np.random.RandomState(4).randint(0, 1 << 40, size=P).astype(np.float64))):
            pool.inst.set_pattern_weights(w)
            pool.w, pool.ref = w, {}
            got = pool.check(tri, keep=2, what=what)
            assert (got == 0).all() if what == "zeros" else (got > (1 << 32)).all()
    finally:
        pool.close()
    # a weight that is not an integer: refused, with the edge call's message, and nothing ran -- no kept candidate
    w = np.ones(P); w[100] = 2.5
    pool = Pool(P, ns, general, 22, wght=w)
    try:
        assert _code(pool.inst.regraft_parsimony, [(0, 1, 2)], keep=0) == capi.ERROR_NO_IMPLEMENTATION
        with pytest.raises(capi.PhyhipError, match="a pattern weight is not an integer"):
            pool.inst.regraft_parsimony([(0, 1, 2)], keep=0)
        with pytest.raises(capi.PhyhipError, match="a pattern weight is not an integer"):
            pool.inst.edge_parsimony(0, 1)
        assert _code(pool.inst.regraft_site_parsimony) == capi.ERROR_OUT_OF_RANGE
        assert _code(pool.inst.regraft_partial_parsimony, general=general) == capi.ERROR_OUT_OF_RANGE
        pool.inst.set_pattern_weights(np.ones(P))                # whole numbers again: served
        pool.w, pool.ref = np.ones(P), {}
        pool.check([(0, 1, 2), (7, 8, 3)], keep=1, what="weights set again")
    finally:
        pool.close()


# ---- 6. the kept candidate -------------------------------------------------------------------------------------------------------------

def test_kept_candidate():
    from phyml_amd import capi
    pool = Pool(131, 4, False, 33)
    try:
        inst, tri = pool.inst, pool.triples(9, 2)
        assert _code(inst.regraft_site_parsimony) == capi.ERROR_OUT_OF_RANGE                      # before any scan
        assert _code(inst.regraft_partial_parsimony) == capi.ERROR_OUT_OF_RANGE
        pool.check(tri, keep=0, what="first")
        pool.check(tri, keep=len(tri) - 1, what="last")
        assert _code(inst.regraft_partial_parsimony, general=True) == capi.ERROR_OUT_OF_RANGE     # the Fitch mode holds no p_pars
        pool.check(tri, keep=-1, what="none")
        assert _code(inst.regraft_site_parsimony) == capi.ERROR_OUT_OF_RANGE                      # after a scan that kept none
        assert _code(inst.regraft_partial_parsimony) == capi.ERROR_OUT_OF_RANGE
        pool.check(tri, keep=4, what="again")
        assert inst.regraft_parsimony([]).shape == (0,)                                          # count == 0 succeeds
        # a mode switch frees the planes: the kept vector goes with them; the same mode again keeps nothing either
        step = random_step(4, 1)
        inst.set_parsimony(True, step)
        assert _code(inst.regraft_site_parsimony) == capi.ERROR_OUT_OF_RANGE
        assert _code(inst.regraft_partial_parsimony, general=True) == capi.ERROR_OUT_OF_RANGE
        inst.update_partial_parsimony(pool.ops)
        pool.general, pool.step, pool.ref = True, step, {}
        pool.pl = pars_ref.Planes(pool.masks, 4, step).run(pool.ops)
        pool.check(tri, keep=2, what="step matrix after the switch")
        assert _code(inst.regraft_partial_parsimony) == capi.ERROR_OUT_OF_RANGE                   # the step-matrix mode holds no ui / pars
    finally:
        pool.close()


# ---- 7. sharded instances --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general,ns", [(False, 4), (True, 20)])
def test_sharded_instances(general, ns):
    plain = Pool(2 * 256 + 77, ns, general, 61)
    try:
        tri = plain.triples(40, 6)
        want = plain.check(tri, keep=7, what="plain")
        J0, site0 = kept(plain.inst, general)
        for shards in (1, 2, 3):
            pool = Pool(2 * 256 + 77, ns, general, 61, devices=[0] * shards, force_sharded=True)
            try:
                got = pool.check(tri, keep=7, what=shards)
                assert np.array_equal(got, want)
                J, site = kept(pool.inst, general)
                assert same_vector(J, J0, general) and np.array_equal(site, site0)
            finally:
                pool.close()
    finally:
        plain.close()


# ---- 8. isolation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
def test_a_scan_leaves_the_parsimony_state_alone(general):
    pool = Pool(300, 4, general, 71)
    try:
        inst, T = pool.inst, pool.T
        l, r = T.left_idx[2], T.rght_idx[2]
        c = inst.edge_parsimony(l, r)
        site = inst.site_parsimony()
        get = (lambda b: inst.partial_parsimony(b, general=True)) if general else inst.partial_parsimony
        before = [get(b) for b in range(pool.n, T.nbuf + 1)]
        inst.profile(1)
        inst.profile_read_parsimony()
        tri = pool.triples(20, 8)
        pool.check(tri, keep=3, what="scan")
        pool.check(tri * 40, keep=-1, what="a longer scan")
        assert inst.profile_read_parsimony() == (0.0, 0, 0.0)           # no launch of the operation lists' kernels, nothing counted
        inst.profile(0)
        assert np.array_equal(inst.site_parsimony(), site)              # of the last scored edge
        for b, want in zip(range(pool.n, T.nbuf + 1), before):
            assert same_vector(get(b), want, general), b
        assert inst.edge_parsimony(l, r) == c
    finally:
        pool.close()


def _likelihood_run(with_scans):
    from gpu_common import synthetic_pair
    t, ot, tree, st = synthetic_pair(26, 150, 4, 4, seed=6, ambiguous_every=6)
    try:
        t.Set_Both_Sides(True)
        first = t.Lk(None)
        b5 = t.Lk(5)
        t.Make_Tree_For_Pars(False)
        t.Set_Both_Sides(True)
        t.Pars(None)
        t.Update_All_Partial_Lk()                      # likelihood operations queued and not launched
        stats = t.inst.virtual_stats()
        if with_scans:
            targets = [e for e in range(2 * 26 - 3) if e != 7]
            t.Pars_Regraft_Scan(7, int(tree.edge_left[7]), targets, keep=3)
            t.Get_Regraft_Site_Pars()
            t.Make_Tree_For_Pars(True)
            t.Pars(None)
            t.Pars_Regraft_Scan(7, int(tree.edge_rght[7]), targets)
            t.inst.profile_read_regraft_parsimony()
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


# ---- 9. errors and profile counters ----------------------------------------------------------------------------------------------------

def test_errors():
    import ctypes as C
    from phyml_amd import capi
    n, P, ns = 4, 20, 4
    masks = random_masks(n, P, ns, 1)
    inst = make_instance(masks, ns, n + 4)
    try:
        for fn, args in ((inst.regraft_parsimony, ([(0, 1, 2)],)), (inst.regraft_parsimony, ([],)), (inst.regraft_site_parsimony, ()),
                         (inst.regraft_partial_parsimony, ()), (inst.profile_read_regraft_parsimony, ())):
            assert _code(fn, *args) == capi.ERROR_UNINITIALIZED_INSTANCE, fn      # before phyhip_set_parsimony
        inst.set_parsimony(False)
        inst.update_partial_parsimony([(n, 0, 1)])
        good = (n, 2, 3)
        for bad in ((-1, 2, 3), (n + 4, 2, 3), (n, -1, 3), (n, n + 4, 3), (n, 2, -1), (n, 2, n + 4)):
            assert _code(inst.regraft_parsimony, [good, bad], keep=0) == capi.ERROR_OUT_OF_RANGE, bad
        for keep in (-2, 2, 100):
            assert _code(inst.regraft_parsimony, [good, good], keep=keep) == capi.ERROR_OUT_OF_RANGE, keep
        assert _code(inst.regraft_parsimony, [], keep=0) == capi.ERROR_OUT_OF_RANGE
        arr = (capi.ParsimonyCandidate * 1)(capi.ParsimonyCandidate(*good))
        out = (C.c_longlong * 1)()
        L = inst.L
        assert L.phyhip_calculate_regraft_parsimony(inst.id, None, 1, -1, out) == capi.ERROR_OUT_OF_RANGE      # NULL arrays with count > 0
        assert L.phyhip_calculate_regraft_parsimony(inst.id, arr, 1, -1, None) == capi.ERROR_OUT_OF_RANGE
        assert L.phyhip_calculate_regraft_parsimony(inst.id, arr, -1, -1, out) == capi.ERROR_OUT_OF_RANGE
        assert L.phyhip_calculate_regraft_parsimony(inst.id, None, 0, -1, None) == 0                           # count == 0 succeeds
        assert L.phyhip_get_regraft_site_parsimony(inst.id, None) == capi.ERROR_OUT_OF_RANGE
        # nothing of the refused calls ran or was kept; what was queued before them is still seen by the call that is served
        assert _code(inst.regraft_site_parsimony) == capi.ERROR_OUT_OF_RANGE
        pl = pars_ref.Planes(masks, ns).run([(n, 0, 1)])
        J, site = rr.join_and_score(pl, n + 3, good)
        assert int(inst.regraft_parsimony([good], keep=0)[0]) == int(site.sum())
        assert np.array_equal(inst.regraft_site_parsimony(), site)
    finally:
        inst.close()
    cls = capi.Instance(4, 10, 4, 16, 5, 4, device=0, class_axis=True)
    try:
        assert _code(cls.regraft_parsimony, [(0, 1, 2)]) == capi.ERROR_NO_IMPLEMENTATION
        assert _code(cls.regraft_site_parsimony) == capi.ERROR_NO_IMPLEMENTATION
    finally:
        cls.close()
    rank = make_instance(masks, ns, n + 4)
    try:
        rank.comm_init_rank(1, 0, capi.comm_get_unique_id())
        assert _code(rank.regraft_parsimony, [(0, 1, 2)]) == capi.ERROR_NO_IMPLEMENTATION
    finally:
        rank.close()
    # (the refusal of other state counts is shared with the six other parsimony calls and cannot be reached: no instance of another
    # state count can be created, tests/test_gpu_cases.py)


def test_profile_counters():
    pool = Pool(300, 4, False, 81)
    try:
        inst, tri = pool.inst, pool.triples(10, 1)
        inst.regraft_parsimony(tri)                               # not profiled: not counted
        inst.profile(1)
        assert inst.profile_read_regraft_parsimony() == (0.0, 0, 0)
        inst.regraft_parsimony(tri)
        inst.regraft_parsimony(tri * 7, keep=5)
        inst.regraft_parsimony([])
        ms, calls, cands = inst.profile_read_regraft_parsimony()
        assert calls == 2 and cands == 80 and ms > 0.0
        assert inst.profile_read_regraft_parsimony() == (0.0, 0, 0)   # reading resets
        # queued operations run in front of a scan as a launch of the operation lists, and are counted there
        inst.update_partial_parsimony(pool.ops)
        inst.regraft_parsimony(tri)
        assert inst.profile_read_parsimony()[1:] == (1, float(pool.P * len(pool.ops)))
        assert inst.profile_read_regraft_parsimony()[1:] == (1, 10)
        inst.profile(0)
    finally:
        pool.close()


# ---- 10. the host layer ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("case", ["designed_nt", "designed_aa"])
def test_host_layer_resolves_the_indices(case, general):
    """Pars_Regraft_Scan on the intact tree against the device's per-candidate route (one queued operation into the spare buffer and
    the edge score) on a second, identical tree, with indices the test resolves from the topology itself: index resolution, not
    arithmetic"""
    base, _ = rr.load(case)
    ns, n, E = int(base["ns"][0]), int(base["n_otu"][0]), len(base["edge_left"])
    t, t2 = lk_tree(base), lk_tree(base)
    try:
        for x in (t, t2):
            x.Make_Tree_For_Pars(general, base["step_mat"] if (general and ns == 20) else None)
            x.Set_Both_Sides(True)
            x.Pars(None)
        c_pars, site_pars = t.c_pars, t.site_pars
        side = lambda x, e, s: (int((base["edge_left"], base["edge_rght"])[s][e]) if (base["edge_left"], base["edge_rght"])[s][e] < n
                                else x.side_buffer(e, s))
        for b_sub in range(E):
            for s in (0, 1):
                d_sub = int((base["edge_left"], base["edge_rght"])[s][b_sub])
                targets = [e for e in range(E) if e != b_sub]
                got = t.Pars_Regraft_Scan(b_sub, d_sub, targets, keep=len(targets) // 2)
                kept_site = t.Get_Regraft_Site_Pars()
                for i, e in enumerate(targets):
                    t2.inst.update_partial_parsimony([(t2.spare_p_lk_idx, side(t2, e, 0), side(t2, e, 1))])
                    assert int(got[i]) == t2.inst.edge_parsimony(t2.spare_p_lk_idx, side(t2, b_sub, s)), (case, b_sub, s, e)
                    if i == len(targets) // 2:
                        assert np.array_equal(kept_site, t2.inst.site_parsimony())
                        J = t.Get_Regraft_Partial_Pars()
                        assert same_vector(J, t2.inst.partial_parsimony(t2.spare_p_lk_idx, general=general), general)
        assert t.c_pars == c_pars and np.array_equal(t.site_pars, site_pars)      # tree->c_pars and tree->site_pars are left alone
    finally:
        t.close()
        t2.close()
