"""phyhip_calculate_mixture_regraft_log_likelihoods (phyml_amd/csrc/phyhip_regraft.hip; MIXT_Lk_Regraft_Scan in the host layer): K
regraft candidates of one pruned subtree over every class tree of a mixture in one device call.

The reference of every value is tests/mixture_regraft_common.py: per class the CPU oracle at buffer level (orc_update_partial into a
spare vector, then orc_edge_lnl, whose unscaled_site_lk_cat / fact_sum_scale outputs are x_k and f_k), combined by
phyml_amd.replay.mixture_combine; tests/test_mixture_regraft_restatement.py pins that pipeline to the real PhyML's dumps, exactly.

Held for every candidate: |lnL - ref| <= 1e-11 |ref| (BAR of tests/test_gpu_regraft.py, for its reasons: every term is a weighted log
of a positive number of one sign, nothing cancels); per class the three matrices and the kept vector with its exponents are the
oracle's (np.array_equal, the vector at patterns with weight, rows without weight zero); the warning equals the restatement's.  The
per-candidate device route -- in every class instance phyhip_update_transition_matrices and phyhip_update_partials into the spare
buffer, then one phyhip_calculate_mixture_log_likelihood -- runs beside the scan and is held to the same bar.  Two device results of
the scan compare with `==`.

Class models: replay.mixture_classes of tests/golden/mixture_nt4.phyg (four nucleotide classes) and mixture_lg4x.phyg (the four LG4X
classes); trees and alignments: the regraft tests' small synthetic shapes, every fifth site of every tip ambiguous, both sides
evaluated.  At these shapes every natural exponent is 0: the rescaling paths are reached with planted exponents."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mixture_regraft_common as mrc
from gpu_common import assert_device_state_is_the_oracles, synthetic_oracle
from mixture_regraft_common import LEFT, within_bar
from phyml_amd import capi, lktree, replay
from test_gpu_regraft import raw_records

FIXTURE_OF = {4: "nt4", 20: "lg4x"}
SMALL_SHAPES = {4: (9, 300), 20: (7, 270)}
SEED = 3
WHO = "phyhip_calculate_mixture_regraft_log_likelihoods"


class Mixture:
    """The class trees of a mixture on the device with their oracle trees: the same topology, lengths and alignment in every class"""

    def __init__(self, models, factors, sums, n, el, er, ln, wght, tv, ds, amb, apply_scaling=1, host_pmat=True, devices=None,
                 force_sharded=False, evaluate=True):
        S, P = int(models[0]["ns"][0]), len(wght)
        self.factors, self.sums, self.K = factors, sums, len(models)
        self.ots = mrc.class_oracles(models, n, el, er, ln, wght, tv, ds, amb, apply_scaling)
        self.trees = []
        try:
            for md in models:
                t = lktree.LkTree(n, el, er, ln, P, S, 1, host_pmat=host_pmat, devices=devices, force_sharded=force_sharded)
                self.trees.append(t)
                t.tip_root = 0   # src/mixt.c:889
                t.set_model(md["pi"], md["gamma_rr"], md["gamma_r_proba"], md["e_val"], md["r_e_vect"], md["l_e_vect"], float(md["l_min"][0]),
                            float(md["l_max"][0]), float(md["br_len_mult"][0]), apply_scaling, 0, 0.0)
                t.Make_Tree_For_Lk(wght, None)
                t.set_tips(tip_partials=tv)
                t.Set_Both_Sides(True)
                if evaluate:
                    t.Lk(None)
            if evaluate:
                for ot in self.ots:
                    ot.lk(None, both_sides=True)
        except Exception:
            self.close()
            raise
        self.ids = [t.tree.contents.b_inst for t in self.trees]
        self.first = self.trees[0].inst
        self.invariant = None

    @classmethod
    def synthetic(cls, ns, P=None, K=4, n=None, seed=SEED, wght=None, lmin=0.02, lmax=0.3, **kw):
        d, models, factors, sums = mrc.fixture(FIXTURE_OF[ns])
        n = SMALL_SHAPES[ns][0] if n is None else n
        P = SMALL_SHAPES[ns][1] if P is None else P
        ot0, tree, st, tv, wg = synthetic_oracle(n, P, ns, 1, seed, lmin, lmax, wght, 1, 5)
        pick = [k % len(models) for k in range(K)]     # more classes than the fixture has: its classes over again
        models, factors = [models[k] for k in pick], [factors[k] for k in pick]
        M = cls(models[:K], factors[:K], sums, n, tree.edge_left, tree.edge_rght, tree.edge_len, wg, ot0.tip_vec, ot0.tip_ds, ot0.tip_amb, **kw)
        M.tree = tree
        return M

    def close(self):
        for t in self.trees:
            t.close()

    def coef(self, order=None):
        f = self.factors if order is None else [self.factors[k] for k in order]
        return [x[0] for x in f], [x[1] for x in f], [x[2] for x in f], self.sums[0], self.sums[1], self.sums[2]

    def scan(self, cands, keep=-1, with_warnings=False, order=None):
        ids = self.ids if order is None else [self.ids[k] for k in order]
        return capi.mixture_regraft_log_likelihoods(ids, None, cands, *self.coef(order), keep=keep, with_warnings=with_warnings)

    def checkers(self):
        return [mrc.ClassChecker(ot, {t.side_buffer(e, side): (ot.plk[(e, side)], ot.scale[(e, side)]) for (e, side) in ot.plk})
                for t, ot in zip(self.trees, self.ots)]

    def reference(self, chks, cand):
        return mrc.mixture_candidate(chks, self.factors, self.sums, cand, self.invariant)

    def set_invariant(self, pinvar, invar, pi_inv):
        invar = np.ascontiguousarray(invar, dtype=np.int16); pi_inv = np.ascontiguousarray(pi_inv, dtype=np.float64)
        capi._chk(self.first.L.phyhip_set_mixture_invariant_sites(self.ids[0], 1, C.c_double(pinvar), capi._ptr(invar), capi._ptr(pi_inv)))
        self.invariant = (pinvar, invar, pi_inv)

    def route(self, cand):
        """The per-candidate device route: (lnL, warning)"""
        c1, c2, sub, flags, l1, l2, l3 = cand
        par, chi, pms = [], [], []
        for t in self.trees:
            spare, sm = t.spare_p_lk_idx, t.spare_Pij_idx
            t.inst.update_transition_matrices([sm, sm + 1, sm + 2], [l1, l2, l3])
            t.inst.update_partials([(spare, c1, sm, c2, sm + 1)])
            par.append(sub if flags & LEFT else spare); chi.append(spare if flags & LEFT else sub); pms.append(sm + 2)
        return capi.mixture_log_likelihood(self.ids, par, chi, pms, *self.coef()), self.first.numerical_warning()


def check_scan(M, chks, cands, keeps, what=None, matrices=True, route=True):
    """One scan per entry of `keeps` (-1: nothing kept), every candidate held to the reference; returns the log-likelihoods"""
    w = M.ots[0].wght > 0
    refs = [M.reference(chks, c) for c in cands]
    first = None
    for n_keep, keep in enumerate(keeps):
        lnl, warn = M.scan(cands, keep=keep, with_warnings=True)
        if first is None:
            first = lnl
        assert np.array_equal(lnl, first), (what, "the kept candidate changed a sum")
        for k, (c, r) in enumerate(zip(cands, refs)):
            assert within_bar(lnl[k], r[0]), (what, k, c, lnl[k], r[0], abs(lnl[k] - r[0]) / abs(r[0]))
            assert warn[k] == r[1], (what, k, c, warn[k], r[1])
            if matrices and n_keep == 0:
                for cl in range(M.K):
                    for which in range(3):
                        assert np.array_equal(M.first.mixture_regraft_transition_matrix(cl, k, which), r[2][cl][4][which]), (what, k, cl, which)
        if keep >= 0:
            for cl in range(M.K):
                vec, sc = M.first.mixture_regraft_partials(cl)
                assert np.array_equal(vec[w], refs[keep][2][cl][2][w]), (what, "kept vector", keep, cl, cands[keep])
                assert np.array_equal(sc[w], refs[keep][2][cl][3][w]), (what, "kept exponents", keep, cl, cands[keep])
                assert not np.any(vec[~w]) and not np.any(sc[~w])
    worst = max(abs(a - r[0]) / abs(r[0]) for a, r in zip(first, refs))
    print(what, "K =", len(cands), "worst relative difference of the scan to the reference:", worst)
    if route:
        for k, (c, r) in enumerate(zip(cands, refs)):
            v, wn = M.route(c)
            print("   candidate", k, "per-candidate route", repr(v), "scan", repr(first[k]), "reference", repr(r[0]))
            assert within_bar(v, r[0]) and wn == r[1], (what, "per-candidate route", k, v, r[0], wn, r[1])
    return first


@pytest.fixture(scope="module")
def small():
    """The small shapes with four classes, 37 raw records and their scan: shared and left unchanged."""
    cache = {}

    def get(ns):
        if ns not in cache:
            M = Mixture.synthetic(ns)
            cands = raw_records(M.trees[0], M.ots[0], 37, seed=17 + ns)
            cache[ns] = (M, cands, M.scan(cands))
        return cache[ns]
    yield get
    for v in cache.values():
        v[0].close()


# 1. small shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,P,K", [(4, 300, 1), (4, 300, 2), (4, 300, 4), (4, 1, 4), (4, 255, 4), (4, 256, 4), (4, 257, 4),
                                    (20, 270, 1), (20, 270, 2), (20, 270, 4),
                                    (4, 300, 3), (4, 300, 5), (20, 270, 3), (20, 270, 5)])   # class counts that are no power of two
def test_small_shapes(ns, P, K):
    M = Mixture.synthetic(ns, P, K)
    try:
        chks, ot = M.checkers(), M.ots[0]
        cands = raw_records(M.trees[0], ot, 37, seed=100 * ns + K)
        assert {(c[0] < ot.n, c[1] < ot.n) for c in cands} == {(False, False), (True, False), (False, True), (True, True)}
        assert {(c[2] < ot.n, c[3]) for c in cands} == {(False, 0), (True, 0), (False, LEFT)}
        assert any(c[4] == 0.0 for c in cands) and any(c[5] < 0.0 for c in cands) and any(c[6] == c[4] for c in cands)
        check_scan(M, chks, cands[:1], [0], (ns, P, K, "K=1"))
        check_scan(M, chks, cands[1:3], [0, 1], (ns, P, K, "K=2"))
        check_scan(M, chks, cands[3:7], [0, 1, 2, 3], (ns, P, K, "K=4"), route=False)
        check_scan(M, chks, cands, [-1, 0, 18, 36], (ns, P, K, "K=37"), route=False)
    finally:
        M.close()


# 2. the real reference's number ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", ["nt4", "lg4x"])
def test_the_in_place_candidate_is_the_references_mixture_lnl(fx):
    d, models, factors, sums = mrc.fixture(fx)
    n, S = int(d["n_otu"][0]), int(d["ns"][0])
    tv, ds, amb = replay.tips_from_masks(d["tip_mask"], S)
    M = Mixture(models, factors, sums, n, d["edge_left"], d["edge_rght"], d["edge_len"], d["wght"], tv, ds, amb)
    try:
        e = int(d["eval_edge"][0])
        assert e == M.ots[0].root_edge()
        t0 = M.trees[0]
        cand = mrc.in_place_candidate(M.ots[0], t0.side_buffer)
        ref = float(d["lnL"][0])
        got = check_scan(M, M.checkers(), [cand], [0], fx)[0]
        assert within_bar(got, ref), (got, ref)
        own = capi.mixture_log_likelihood(M.ids, [t.side_buffer(e, 0) for t in M.trees], [int(M.ots[0].er[e])] * M.K,
                                          [t.edge(e).contents.Pij_rr_idx for t in M.trees], *M.coef())
        assert within_bar(own, ref) and within_bar(got, own), (got, own, ref)
    finally:
        M.close()


# 3. planted exponents ------------------------------------------------------------------------------------------------------------------
def plant(M, chks, idx, exponents=None, factor=None):
    """exponents {class: {pattern: value}} set in buffer idx of the class instances (phyhip_set_scale_factors) and in the checkers'
    buffers; factor {pattern: multiplier} applied to the partials of every class"""
    for cl, (t, chk) in enumerate(zip(M.trees, chks)):
        p, sc = chk.buf[idx]
        p, sc = p.copy(), sc.copy()
        for pat, v in (exponents or {}).get(cl, {}).items():
            sc[pat] = v
        for pat, v in (factor or {}).items():
            p[pat] *= v
        chk.buf[idx] = (p, sc)
        t.inst.set_partials(idx, p)
        capi._chk(t.inst.L.phyhip_set_scale_factors(t.inst.id, idx, capi._ptr(sc)))


@pytest.mark.parametrize("ns", [4, 20])
def test_planted_exponents(ns):
    M = Mixture.synthetic(ns)
    try:
        chks = M.checkers()
        assert all(not np.any(sc) for chk in chks for (p, sc) in chk.buf.values())            # every natural exponent is 0
        a, b, c, d1, d2, d3, d4 = sorted(chks[0].buf)[:7]
        K = M.K
        small = range(10, 20)
        plant(M, chks, a, {cl: {p: v for p in small} for cl, v in enumerate((0, 2, 5, 8))}, {p: 1e-80 for p in range(30, 35)})
        plant(M, chks, b, {cl: {p: v for p in range(15, 25)} for cl, v in enumerate((8, 0, 2, 5))}, {p: 1e-80 for p in range(30, 35)})
        plant(M, chks, c, {cl: {12: 256 * cl} for cl in range(K)})
        plant(M, chks, d1, {1: {40: 1024}})                                   # one class at exactly 1024: it drops out
        plant(M, chks, d2, {cl: {41: 1024} for cl in range(K)})               # ... every class: the floor
        plant(M, chks, d3, {2: {42: 1030}})                                   # one class above 1024: the cap and the warning
        plant(M, chks, d4, {cl: {43: 1000 + 30 * (cl + 1)} for cl in range(K)})   # ... every class
        cands = [(a, b, c, 0, 0.1, 0.2, 0.3), (a, 2, c, LEFT, 0.2, 0.1, 0.05), (d1, b, c, 0, 0.1, 0.2, 0.3), (d2, 3, c, 0, 0.1, 0.2, 0.3),
                 (d3, 1, 4, 0, 0.1, 0.2, 0.3), (b, d4, c, LEFT, 0.3, 0.1, 0.2)]
        refs = [M.reference(chks, x) for x in cands]
        f = lambda k, cl: refs[k][2][cl][1]
        assert [int(f(0, cl)[11]) for cl in range(K)] == [0, 2, 5, 8]                  # sums that differ a little: every class matters
        assert [int(f(0, cl)[17]) for cl in range(K)] == [8, 2, 7, 13]
        own = refs[0][2][0][3] - chks[0].buf[a][1] - chks[0].buf[b][1]
        assert np.all(own[30:35] == 256) and not np.any(own[:30])                       # the 2^256 rule
        assert f(2, 1)[40] == 1024 and all(f(2, cl)[40] == 0 for cl in (0, 2, 3))
        assert all(f(3, cl)[41] == 1024 for cl in range(K))
        assert f(4, 2)[42] == 1030 and all(f(5, cl)[43] > 1024 for cl in range(K))
        assert [r[1] for r in refs] == [0, 0, 0, 1, 1, 1]
        check_scan(M, chks, cands, list(range(len(cands))), ("planted exponents", ns))
    finally:
        M.close()


# 4. zero-weight patterns, +I, the floor, no scaling -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_zero_weight_patterns_and_an_invariant_class(ns):
    P = SMALL_SHAPES[ns][1]
    wght = np.where(np.arange(P) % 7 == 3, 0.0, 1.0 + (np.arange(P) % 3))
    M = Mixture.synthetic(ns, wght=wght)
    try:
        chks = M.checkers()
        cands = raw_records(M.trees[0], M.ots[0], 16, seed=9)
        plain = check_scan(M, chks, cands, [-1, 0, 7, 15], ("zero weights", ns), route=False)
        check_scan(M, chks, cands[:3], [0], ("zero weights", ns))
        pi_inv = np.asarray(M.ots[0].m.pi)
        M.set_invariant(0.2, np.where(np.arange(P) % 3 == 0, np.arange(P) % ns, -1), pi_inv)
        with_i = check_scan(M, chks, cands, [-1, 5], ("+I", ns), route=False)
        check_scan(M, chks, cands[:3], [1], ("+I", ns))
        assert not np.any(with_i == plain)
    finally:
        M.close()


def test_small_floor_raises_the_candidates_own_warning():
    M = Mixture.synthetic(4)
    try:
        chks = M.checkers()
        a, b, c, e = sorted(chks[0].buf)[:4]
        for idx in (a, b):
            plant(M, chks, idx, factor={p: 1e-200 for p in range(1, M.ots[0].P, 7)})
        assert M.first.numerical_warning() == 0
        cands = [(a, b, c, 0, 0.1, 0.2, 0.3), (c, e, 0, 0, 0.1, 0.2, 0.3), (a, b, c, LEFT, 0.2, 0.1, 0.05), (a, 2, 4, 0, 0.1, 0.1, 0.1)]
        refs = [M.reference(chks, x) for x in cands]
        assert [r[1] for r in refs] == [1, 0, 1, 0]
        check_scan(M, chks, cands, [0, 1, 2, 3], "SMALL floor", route=False)
        assert all(t.inst.numerical_warning() == 0 for t in M.trees)
    finally:
        M.close()


def test_without_lk_scaling():
    M = Mixture.synthetic(4, P=40, K=2, n=120, seed=5, lmin=1.0, lmax=3.0, apply_scaling=0)
    try:
        chks = M.checkers()
        cands = raw_records(M.trees[0], M.ots[0], 8, seed=4)
        refs = [M.reference(chks, c) for c in cands]
        assert all(not np.any(cl[1]) and not np.any(cl[3]) for r in refs for cl in r[2])                  # no exponent anywhere
        assert any(0.0 < cl[2][cl[2] > 0].min() < 2.0 ** -256 for r in refs for cl in r[2])               # ... where scaling would have stepped in
        check_scan(M, chks, cands, [0, 3, 7], "apply_lk_scaling = 0", route=False)
    finally:
        M.close()


# 5. bits that must not move --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_a_candidates_bits_depend_on_the_candidate_and_the_class_list_alone(ns, small):
    M, cands, base = small(ns)
    assert np.array_equal(M.scan(cands), base)                                      # the same call twice
    for k in (0, 18, 36):                                                           # first, middle, last of 37 -- and alone
        assert M.scan([cands[k]])[0] == base[k]
    perm = np.random.default_rng(1).permutation(len(cands))
    got = M.scan([cands[i] for i in perm])
    assert all(got[j] == base[i] for j, i in enumerate(perm))
    P = M.ots[0].P
    fixed = M.K * (P * ns * 8 + ((P + 1) // 2 * 2) * 4 + 128) + 200
    per = 3 * M.K * ns * ns * 8 + (P + 255) // 256 * 8 + 72
    w = M.ots[0].wght > 0
    try:
        for chunk in (1, 5):
            bound = fixed + chunk * per + per // 2
            assert capi.mixture_regraft_chunk_candidates(P, M.K, ns, bound) == chunk
            M.first.set_mixture_regraft_work_space(bound)
            assert np.array_equal(M.scan(cands, keep=5), base), chunk
            ref = M.reference(M.checkers(), cands[5])
            for cl in range(M.K):                                                   # kept in an early chunk, read after the last
                vec, sc = M.first.mixture_regraft_partials(cl)
                assert np.array_equal(vec[w], ref[2][cl][2][w]) and np.array_equal(sc[w], ref[2][cl][3][w])
            last = M.reference(M.checkers(), cands[36])
            assert np.array_equal(M.first.mixture_regraft_transition_matrix(M.K - 1, 36, 2), last[2][M.K - 1][4][2])   # the last chunk's are there
            with pytest.raises(capi.PhyhipError) as ei:
                M.first.mixture_regraft_transition_matrix(0, 0, 0)                  # an earlier chunk's have left
            assert ei.value.code == capi.ERROR_OUT_OF_RANGE
    finally:
        M.first.set_mixture_regraft_work_space(0)
    # after unrelated calls: a plain scan of a class instance, an evaluation of another
    M.trees[1].inst.regraft_log_likelihoods(cands[:3], keep=1)
    M.trees[2].Lk(None)
    assert np.array_equal(M.scan(cands), base)
    # another order of the classes (with their tables) is another sum per pattern: its bits may differ, and nothing is claimed
    order = [2, 0, 3, 1]
    other = M.scan(cands, order=order)
    print("classes permuted:", int((other != base).sum()), "of", len(cands), "candidates differ in bits; worst relative difference",
          float(np.max(np.abs(other - base) / np.abs(base))))
    assert all(within_bar(x, y) for x, y in zip(other, base))


# 6. isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_a_scan_changes_nothing_but_its_work_space(ns):
    M = Mixture.synthetic(ns)
    try:
        ot = M.ots[0]
        e = next(k for k in range(ot.ne) if ot.el[k] >= ot.n and ot.er[k] >= ot.n)
        for t, o in zip(M.trees, M.ots):
            t.Update_Eigen_Lr(e)
            t.Lk(e); o.lk(e)
        cands = raw_records(M.trees[0], ot, 12, seed=8)
        plain = M.trees[1].inst.regraft_log_likelihoods(cands[:4], keep=2)          # a class instance's own plain scan
        kept, pm = M.trees[1].inst.regraft_partials(), M.trees[1].inst.regraft_transition_matrix(3, 1)
        state = lambda: [(t.inst.site_outputs(), t.inst.get_dot_prod(), t.inst.numerical_warning(),
                          [t.inst.get_transition_matrix(k) for k in range(ot.ne + 4)]) for t in M.trees]
        before = state()
        M.scan(cands, keep=4)
        for t, o in zip(M.trees, M.ots):
            assert_device_state_is_the_oracles(t, o, what="after a mixture scan")
        for bf, af in zip(before, state()):
            assert all(np.array_equal(x, y) for x, y in zip(bf[0], af[0]))
            assert np.array_equal(bf[1], af[1]) and bf[2] == af[2]
            assert all(np.array_equal(x, y) for x, y in zip(bf[3], af[3]))
        again = M.trees[1].inst.regraft_partials()
        assert np.array_equal(again[0], kept[0]) and np.array_equal(again[1], kept[1])
        assert np.array_equal(M.trees[1].inst.regraft_transition_matrix(3, 1), pm)
        assert np.array_equal(M.trees[1].inst.regraft_log_likelihoods(cands[:4]), plain)
    finally:
        M.close()


# 7. streams and queues -----------------------------------------------------------------------------------------------------------------
def test_a_queued_path_update_in_every_class_is_seen():
    M = Mixture.synthetic(4)
    try:
        ot0 = M.ots[0]
        e = next(k for k in range(ot0.ne) if ot0.el[k] >= ot0.n and ot0.er[k] >= ot0.n)
        d = int(ot0.el[e])
        nb = next(be for (v, be) in ot0.adj[d] if be != e)
        for t, ot in zip(M.trees, M.ots):
            ot.len[nb] = float(ot.len[nb]) * 3.0 + 0.05
            ot.update_pmat(nb); ot.update_partial(e, d)
            t.edge(nb).contents.l = float(ot.len[nb])
            t.Update_PMat_At_Given_Edge(nb)
            t.Update_Partial_Lk(e, d)                       # queued, not launched
        chks = M.checkers()
        target, other = M.trees[0].side_buffer(e, 0), M.trees[0].side_buffer(e, 1)
        cands = [(target, other, 0, 0, 0.1, 0.2, 0.3), (2, target, other, LEFT, 0.3, 0.1, 0.2)]
        check_scan(M, chks, cands, [0, 1], "queued path update", route=False)
        for t, ot in zip(M.trees, M.ots):
            assert_device_state_is_the_oracles(t, ot, what="the queued update ran")
    finally:
        M.close()


@pytest.mark.parametrize("ns,P", [(4, 150), (20, 40)])
def test_virtual_buffers_are_stored_for_the_call(ns, P):
    got = {}
    for virtual in (True, False):
        M = Mixture.synthetic(ns, P=P, K=2, n=26, seed=6, evaluate=False)
        try:
            for t in M.trees:
                if not virtual:
                    t.inst.set_virtual_buffers(0)
                t.Lk(None)
            for ot in M.ots:
                ot.lk(None, both_sides=True)
            now = [t.inst.virtual_stats()[0] for t in M.trees]
            assert all((v > 0) == virtual for v in now), now
            cands = raw_records(M.trees[0], M.ots[0], 24, seed=12)
            got[virtual] = M.scan(cands)
            if virtual:
                assert all(t.inst.virtual_stats()[0] < v and t.inst.virtual_stats()[3] > 0 for t, v in zip(M.trees, now))
            chks = M.checkers()
            assert all(within_bar(v, M.reference(chks, c)[0]) for v, c in zip(got[virtual], cands))
        finally:
            M.close()
    assert np.array_equal(got[True], got[False])


def test_lk_and_dlk_after_a_scan_are_served_resident_again():
    M = Mixture.synthetic(4, P=382, K=2, n=14, seed=23)
    try:
        e = 3
        cands = raw_records(M.trees[0], M.ots[0], 20, seed=3)
        for k, t in enumerate(M.trees):
            t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
            t.Lk(e)
            t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
            chain = lambda: [t.dLk(0.003 * (i + 1), e) for i in range(6)]
            first = chain()
            served, _, _, instead = t.inst.resident_stats(0)
            if k == 0:
                assert served > 0
            M.scan(cands, keep=2)
            again = chain()
            assert first == again
            now = t.inst.resident_stats(0)
            print("class", k, "dLk served resident before / after the scan:", served, now[0] - served)
            if served > 0:                                  # where the resident workgroups served dLk, they serve it again
                assert now[0] == served + len(again) and now[3] == instead, (served, instead, now)
            t.Set_Use_Eigen_Lr(False)
            t.Lk(e)
            s0 = t.inst.resident_stats(1)
            a = t.Lk(e)
            s1 = t.inst.resident_stats(1)
            M.scan(cands)
            b = t.Lk(e)
            s2 = t.inst.resident_stats(1)
            assert a == b
            print("class", k, "Lk(b) served by the short-launch resident evaluator before / after the scan:", s1[0] - s0[0], s2[0] - s1[0])
            if s1[0] == s0[0] + 1:                          # where the short-launch evaluator served Lk(b), it serves it again
                assert s2[0] == s1[0] + 1 and s2[3] == s1[3], (s0, s1, s2)
    finally:
        M.close()


# 8. the error table ----------------------------------------------------------------------------------------------------------------
def _refused(fn, *a, **kw):
    with pytest.raises(capi.PhyhipError) as ei:
        fn(*a, **kw)
    return ei.value.code, str(ei.value)


def test_error_table(small):
    M, cands, base = small(4)
    nbuf = max(M.trees[0].side_buffer(e, s) for (e, s) in M.ots[0].plk) + 1 + 4
    good = cands[0]
    co = M.coef()
    tile = lambda v, n: [v[i % len(v)] for i in range(n)]
    scan = lambda ids, cs, eig=None, **kw: capi.mixture_regraft_log_likelihoods(ids, eig, cs, tile(co[0], len(ids)), tile(co[1], len(ids)),
                                                                                tile(co[2], len(ids)), co[3], co[4], co[5], **kw)
    for c in ((-1,) + good[1:], (good[0], nbuf + 50) + good[2:], good[:2] + (nbuf + 50,) + good[3:], (good[0], good[1], 0, LEFT) + good[4:]):
        code, msg = _refused(scan, M.ids, [good, c])
        assert code == capi.ERROR_OUT_OF_RANGE and WHO in msg, msg
    for kw in (dict(keep=1), dict(keep=7), dict(keep=-2), dict(eig=[0, 1, 0, 0]), dict(eig=[-1, 0, 0, 0])):
        code, msg = _refused(scan, M.ids, [good], **kw)
        assert code == capi.ERROR_OUT_OF_RANGE and WHO in msg, (kw, msg)
    for ids in ([], M.ids * 17):                                                    # count outside 1..64
        code, msg = _refused(capi.mixture_regraft_log_likelihoods, ids, None, [good], [0.1] * len(ids), [1.0] * len(ids), [1.0] * len(ids), 1.0, 1.0, 1.0)
        assert code == capi.ERROR_OUT_OF_RANGE and WHO in msg, msg
    assert np.array_equal(scan(M.ids * 16, [good] * 2).shape, (2,))                 # 64 classes are served
    M.scan(cands)
    first = M.first
    for which in (-1, 3):
        code, msg = _refused(first.mixture_regraft_transition_matrix, 0, 0, which)
        assert code == capi.ERROR_OUT_OF_RANGE and "phyhip_get_mixture_regraft_transition_matrix" in msg
    for cl, k in ((0, len(cands)), (M.K, 0), (-1, 0), (0, -1)):
        assert _refused(first.mixture_regraft_transition_matrix, cl, k, 0)[0] == capi.ERROR_OUT_OF_RANGE
    code, msg = _refused(first.mixture_regraft_partials, 0)                          # the last call kept nothing
    assert code == capi.ERROR_OUT_OF_RANGE and "phyhip_get_mixture_regraft_partials" in msg
    M.scan(cands, keep=3)
    for cl in (-1, M.K):
        assert _refused(first.mixture_regraft_partials, cl)[0] == capi.ERROR_OUT_OF_RANGE
    # a getter on an instance that was never the first of a scan
    for fn, a, name in ((M.trees[1].inst.mixture_regraft_partials, (0,), "phyhip_get_mixture_regraft_partials"),
                        (M.trees[1].inst.mixture_regraft_transition_matrix, (0, 0, 0), "phyhip_get_mixture_regraft_transition_matrix")):
        code, msg = _refused(fn, *a)
        assert code == capi.ERROR_OUT_OF_RANGE and name in msg, msg
    assert M.trees[1].inst.profile_read_mixture_regraft() == (0.0, 0, 0)
    assert M.scan([]).size == 0                                                      # candidateCount == 0 succeeds and does nothing
    assert np.array_equal(M.scan(cands), base)                                       # ... and the instances are still usable
    # refusals by kind of instance, differing shapes: the first class is a good one, the second is not
    rec = [(4, 5, 6, 0, 0.1, 0.1, 0.1)]
    two = lambda x: capi.mixture_regraft_log_likelihoods([ok.id, x.id], None, rec, [0.5, 0.5], [1.0, 1.0], [1.0, 1.0], 2.0, 2.0, 1.0)
    ok = capi.Instance(4, 10, 4, 16, 5, 1)
    try:
        for make, want in ((lambda: capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True), capi.ERROR_NO_IMPLEMENTATION),
                           (lambda: capi.Instance(4, 10, 4, 16, 5, 4), capi.ERROR_OUT_OF_RANGE),       # more than one category
                           (lambda: capi.Instance(4, 10, 4, 17, 5, 1), capi.ERROR_OUT_OF_RANGE),       # another pattern count
                           (lambda: capi.Instance(4, 10, 20, 16, 5, 1), capi.ERROR_OUT_OF_RANGE),      # another state count
                           (lambda: capi.Instance(5, 11, 4, 16, 5, 1), capi.ERROR_OUT_OF_RANGE),       # another tip count
                           (lambda: capi.Instance(4, 10, 4, 16, 5, 1, devices=[0, 0]), capi.ERROR_OUT_OF_RANGE)):   # sharded beside plain
            x = make()
            try:
                code, msg = _refused(two, x)
                assert code == want and WHO in msg, (want, msg)
            finally:
                x.close()
        rank = capi.Instance(4, 10, 4, 16, 5, 1)
        try:
            rank.comm_init_rank(1, 0, capi.comm_get_unique_id())
            code, msg = _refused(two, rank)
            assert code == capi.ERROR_NO_IMPLEMENTATION and WHO in msg, msg
        finally:
            rank.close()
    finally:
        ok.close()


def test_generic_loop_instances_are_refused():
    from gpu_common import synthetic_pair
    g, _, _, _ = synthetic_pair(6, 40, 4, 1, seed=5, use_m4mod=True)   # the reference's generic loop
    try:
        g.Set_Both_Sides(True); g.Lk(None)
        code, msg = _refused(capi.mixture_regraft_log_likelihoods, [g.tree.contents.b_inst], None, [(0, 1, 2, 0, 0.1, 0.1, 0.1)], [1.0], [1.0], [1.0],
                             1.0, 1.0, 1.0)
        assert code == capi.ERROR_NO_IMPLEMENTATION and WHO in msg, msg
        assert g.Lk(None) < 0.0
    finally:
        g.close()


# 9. profile -----------------------------------------------------------------------------------------------------------------------
def test_profile_counts_calls_and_candidates(small):
    M, cands, base = small(20)
    M.first.profile(1)
    try:
        M.scan(cands)
        M.scan(cands[:5])
        ms, calls, n = M.first.profile_read_mixture_regraft()
        assert ms > 0.0 and calls == 2 and n == len(cands) + 5
        assert M.first.profile_read_mixture_regraft() == (0.0, 0, 0)
    finally:
        M.first.profile(0)


# 10. the host layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_the_host_layers_scan(ns, small):
    M, _, _ = small(ns)
    chks, ot, t0 = M.checkers(), M.ots[0], M.trees[0]
    lnl_before = [t.tree.contents.c_lnL for t in M.trees]
    for b_sub, side in ((0, 1), (ot.ne - 1, 0), (ot.ne // 2, 1)):
        d_sub = int(ot.er[b_sub] if side == 1 else ot.el[b_sub])
        for link_is_left in (True, False):
            if not link_is_left and d_sub < ot.n:
                continue
            targets = [e for e in range(ot.ne) if e != b_sub]
            ll = [0.3 * float(M.tree.edge_len[e]) + 0.001 for e in targets]
            lr = [0.7 * float(M.tree.edge_len[e]) + 0.002 for e in targets]
            l_sub = float(M.tree.edge_len[b_sub]) * 1.5
            got = lktree.Mixture_Regraft_Scan(M.trees, *M.coef(), b_sub, d_sub, link_is_left, l_sub, targets, ll, lr)
            sub = d_sub if d_sub < ot.n else t0.side_buffer(b_sub, side)
            for i, e in enumerate(targets):
                c1 = int(ot.el[e]) if ot.el[e] < ot.n else t0.side_buffer(e, 0)
                c2 = int(ot.er[e]) if ot.er[e] < ot.n else t0.side_buffer(e, 1)
                ref = M.reference(chks, (c1, c2, sub, 0 if link_is_left else LEFT, ll[i], lr[i], l_sub))[0]
                assert within_bar(got[i], ref), ("MIXT_Lk_Regraft_Scan", b_sub, side, link_is_left, e, got[i], ref)
    assert [t.tree.contents.c_lnL for t in M.trees] == lnl_before


# 11. sharded class instances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_three_shards_on_one_device(ns, small):
    M1, cands, base = small(ns)
    chks = M1.checkers()
    refs = [M1.reference(chks, c) for c in cands]
    M1.scan(cands, keep=9)
    kept = [M1.first.mixture_regraft_partials(cl) for cl in range(M1.K)]
    M = Mixture.synthetic(ns, devices=[0, 0, 0])
    try:
        assert all(len(t.inst.shard_ranges()) == 3 for t in M.trees)
        assert all(M.trees[0].side_buffer(e, s) == M1.trees[0].side_buffer(e, s) for (e, s) in M.ots[0].plk)
        lnl, warn = M.scan(cands, keep=9, with_warnings=True)
        for k, r in enumerate(refs):
            assert within_bar(lnl[k], r[0]) and within_bar(lnl[k], base[k]) and warn[k] == r[1], (k, lnl[k], r[0], base[k])
        for cl in range(M.K):
            vec, sc = M.first.mixture_regraft_partials(cl)                           # the shards' kept vectors, concatenated
            assert np.array_equal(vec, kept[cl][0]) and np.array_equal(sc, kept[cl][1])
            assert np.array_equal(M.first.mixture_regraft_transition_matrix(cl, 36, 1), M1.first.mixture_regraft_transition_matrix(cl, 36, 1))
        assert np.array_equal(M.scan(cands), lnl)
        assert M.scan([]).size == 0
    finally:
        M.close()
