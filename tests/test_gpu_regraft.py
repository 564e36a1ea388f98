"""phyhip_calculate_regraft_log_likelihoods (phyml_amd/csrc/phyhip_regraft.hip; Lk_Regraft_Scan in the host layer): K regraft
candidates of one pruned subtree in one device call, against the CPU oracle at buffer level -- orc_update_partial into a spare
vector, then orc_edge_lnl, as tests/replay_oracle.py calls them, with the matrices of orc.pmat_edge.

Held for every candidate: the three matrices and the kept vector with its exponents are the oracle's doubles (np.array_equal, the
vector at patterns with weight); |lnL - ref| <= 1e-11 |ref|, the bar tests/test_gpu_replay.py sets for this call pattern (the lnL
takes the general product at every pattern and the device's summation order: every term is a weighted log of a positive number of
the same sign, so nothing cancels -- P x 2^-53 from the order of the sum plus a few 2^-53 per pattern stays under 1e-13 at these
sizes); the warning equals the oracle's.  The existing two-call route (phyhip_update_partials into a spare buffer, then
phyhip_calculate_edge_log_likelihoods) runs beside it on the same instance, is printed, and is held to the oracle by the same bar.
Equalities between two DEVICE results of the scan (repeats, position, chunks) are `==`."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from conftest import GOLDEN
from gpu_common import assert_device_state_is_the_oracles, device_tree_from_golden, synthetic_pair
from phyml_amd import capi, phyg, replay
from replay_oracle import RecordedReplayer, tree_from_recorded

BAR = 1e-11
LEFT = capi.REGRAFT_SUBTREE_IS_LEFT
SMALL_SHAPES = {4: (9, 300), 20: (7, 270)}   # the ancestral tests' small shapes: cross a 256-lane workgroup, ragged tail
SEED = 3


class Checker:
    """The CPU oracle of a candidate on the vectors a device instance holds: buffers = {device buffer index: (partials, exponents)}
    of the internal buffers; an index below n_otu is the oracle tree's tip."""

    def __init__(self, ot, buffers):
        self.ot, self.buf = ot, buffers

    @classmethod
    def of_tree(cls, t, ot):
        return cls(ot, {t.side_buffer(e, side): (ot.plk[(e, side)], ot.scale[(e, side)]) for (e, side) in ot.plk})

    def side(self, idx):
        ot, s = self.ot, orc.Side()
        if idx < ot.n:
            s.p_lk = orc._p(ot.tip_vec[idx]); s.sum_scale = None; s.is_tip = 1
            s.is_ambigu = orc._p(ot.tip_amb[idx]); s.d_state = orc._p(ot.tip_ds[idx])
        else:
            p, sc = self.buf[idx]
            s.p_lk = orc._p(p); s.sum_scale = orc._p(sc); s.is_tip = 0; s.is_ambigu = None; s.d_state = None
        return s

    def pmat(self, l):
        m = self.ot.m
        return orc.pmat_edge(l, m.ns, m.ncatg, m.gamma_rr, m.br_len_mult, m.l_min, m.l_max, m.r_e_vect, m.l_e_vect, m.e_val)

    def candidate(self, cand):
        """(lnL, warning, computed vector, its exponents, the three matrices) of one record"""
        c1, c2, sub, flags, l1, l2, l3 = cand
        ot, m, L = self.ot, self.ot.m, orc.lib()
        pm = [self.pmat(l1), self.pmat(l2), self.pmat(l3)]
        vec = np.zeros((ot.P, m.ncatg * m.ns)); sc = np.zeros(ot.P, np.int32)
        s1, s2 = self.side(c1), self.side(c2)
        L.orc_update_partial(C.c_int(ot.P), C.c_int(m.ncatg), C.c_int(m.ns), orc._p(ot.wght), C.byref(s1), orc._p(pm[0]), C.byref(s2),
                             orc._p(pm[1]), orc._p(vec), orc._p(sc), C.c_int(ot.apply_scaling), C.c_int(ot.arith))
        comp = orc.Side()
        comp.p_lk = orc._p(vec); comp.sum_scale = orc._p(sc); comp.is_tip = 0; comp.is_ambigu = None; comp.d_state = None
        left, rght = (self.side(sub), comp) if flags & LEFT else (comp, self.side(sub))
        warn = C.c_int(0)
        a, b, c, f = np.zeros(ot.P), np.zeros(ot.P), np.zeros((ot.P, m.ncatg)), np.zeros(ot.P, np.int32)
        lnl = L.orc_edge_lnl(C.c_int(ot.P), C.c_int(m.ncatg), C.c_int(m.ns), orc._p(ot.wght), C.byref(left), C.byref(rght), orc._p(pm[2]),
                             orc._p(m.pi), orc._p(m.gamma_r_proba), C.c_int(m.invar_model), C.c_double(m.pinvar), orc._p(ot.invar),
                             C.c_int(ot.apply_scaling), C.c_int(ot.arith), orc._p(a), orc._p(b), orc._p(c), orc._p(f), C.byref(warn))
        return lnl, warn.value, vec, sc, pm


def within_bar(got, ref):
    return abs(got - ref) <= BAR * abs(ref)


def two_call_route(t, cand):
    """The same candidate through phyhip_update_transition_matrices / phyhip_update_partials / phyhip_calculate_edge_log_likelihoods
    with the tree's spare buffer and spare matrices: (lnL, warning)"""
    c1, c2, sub, flags, l1, l2, l3 = cand
    spare, sm = t.spare_p_lk_idx, t.spare_Pij_idx
    t.inst.update_transition_matrices([sm, sm + 1, sm + 2], [l1, l2, l3])
    t.inst.update_partials([(spare, c1, sm, c2, sm + 1)])
    lnl = t.inst.edge_lnl(sub, spare, sm + 2) if flags & LEFT else t.inst.edge_lnl(spare, sub, sm + 2)
    return lnl, t.inst.numerical_warning()


def check_scan(t, chk, cands, keeps, what=None, matrices=True, two_call=True):
    """One scan per entry of `keeps` (-1: nothing kept), every candidate held to the oracle; returns the log-likelihoods"""
    w = chk.ot.wght > 0
    refs = [chk.candidate(c) for c in cands]
    first = None
    for keep in keeps:
        lnl, warn = t.inst.regraft_log_likelihoods(cands, keep=keep, with_warnings=True)
        if first is None:
            first = lnl
        assert np.array_equal(lnl, first), (what, "the kept candidate changed a sum")
        for k, (c, r) in enumerate(zip(cands, refs)):
            assert within_bar(lnl[k], r[0]), (what, k, c, lnl[k], r[0], abs(lnl[k] - r[0]) / abs(r[0]))
            assert warn[k] == r[1], (what, k, c, warn[k], r[1])
            if matrices:
                for which in range(3):
                    assert np.array_equal(t.inst.regraft_transition_matrix(k, which), r[4][which]), (what, k, which)
        if keep >= 0:
            vec, sc = t.inst.regraft_partials()
            assert np.array_equal(vec[w], refs[keep][2][w]), (what, "kept vector", keep, cands[keep])
            assert np.array_equal(sc[w], refs[keep][3][w]), (what, "kept exponents", keep, cands[keep])
            assert not np.any(vec[~w]) and not np.any(sc[~w])
    worst = max(abs(a - r[0]) / abs(r[0]) for a, r in zip(first, refs))
    print(what, "K =", len(cands), "worst relative difference of the scan to the oracle:", worst)
    if two_call:
        for k, (c, r) in enumerate(zip(cands, refs)):
            v, wn = two_call_route(t, c)
            print("   candidate", k, "two-call route", repr(v), "scan", repr(first[k]), "oracle", repr(r[0]))
            assert within_bar(v, r[0]) and wn == r[1], (what, "two-call route", k, v, r[0])
    return first


def raw_records(t, ot, count, seed):
    """Records that cover every kind of operand: internal x internal, tip x internal (both orders), tip x tip children; the subtree a
    buffer and a tip; the computed vector as the left and as the right operand; a zero and a negative length among the lengths."""
    rng = np.random.default_rng(seed)
    internal = sorted(t.side_buffer(e, side) for (e, side) in ot.plk)
    tips = list(range(ot.n))
    kinds = [("ii", "buf", 0), ("ti", "buf", LEFT), ("it", "tip", 0), ("tt", "buf", 0), ("tt", "tip", 0), ("ii", "buf", LEFT), ("ti", "tip", 0),
             ("tt", "buf", LEFT)]
    out = []
    for k in range(count):
        ch, sb, flags = kinds[k % len(kinds)]
        pick = lambda pool: int(pool[int(rng.integers(len(pool)))])
        c1 = pick(tips) if ch[0] == "t" else pick(internal)
        c2 = pick(tips) if ch[1] == "t" else pick(internal)
        sub = pick(tips) if sb == "tip" else pick(internal)
        l = rng.uniform(0.005, 0.6, 3)
        if k % 11 == 5: l[0] = 0.0
        if k % 13 == 7: l[1] = -0.25     # MAX(0, l), then the clamp to l_min
        if k % 5 == 3: l[2] = l[0]       # identical lengths are built once
        out.append((c1, c2, sub, flags, float(l[0]), float(l[1]), float(l[2])))
    return out


def prepared(n, P, ns, Cc, **kw):
    t, ot, tree, st = synthetic_pair(n, P, ns, Cc, seed=SEED, ambiguous_every=5, **kw)
    t.Set_Both_Sides(True)
    t.Lk(None)
    ot.lk(None, both_sides=True)
    return t, ot, tree


@pytest.fixture(scope="module")
def small():
    """The small shapes at 4 categories, evaluated on both sides, with 37 raw records and their scan: shared and left unchanged."""
    cache = {}

    def get(ns):
        if ns not in cache:
            n, P = SMALL_SHAPES[ns]
            t, ot, tree = prepared(n, P, ns, 4)
            cands = raw_records(t, ot, 37, seed=17 + ns)
            cache[ns] = (t, ot, tree, cands, t.inst.regraft_log_likelihoods(cands))
        return cache[ns]
    yield get
    for v in cache.values():
        v[0].close()


# 1. small shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,P,Cc", [(4, 300, 1), (4, 300, 4), (4, 300, 8), (4, 1, 4), (4, 255, 4), (4, 256, 4), (4, 257, 4),
                                     (20, 270, 1), (20, 270, 4), (20, 270, 8),
                                     # category counts that are no power of two (4 states: the unrolled `if (c < q.C)` of the registers)
                                     (4, 300, 3), (4, 300, 5), (4, 300, 7), (20, 270, 3), (20, 270, 5), (20, 270, 7)])
def test_small_shapes(ns, P, Cc):
    t, ot, tree = prepared(SMALL_SHAPES[ns][0], P, ns, Cc)
    try:
        chk = Checker.of_tree(t, ot)
        cands = raw_records(t, ot, 37, seed=100 * ns + Cc)
        assert {(c[0] < ot.n, c[1] < ot.n) for c in cands} == {(False, False), (True, False), (False, True), (True, True)}
        assert {(c[2] < ot.n, c[3]) for c in cands} == {(False, 0), (True, 0), (False, LEFT)}
        check_scan(t, chk, cands[:1], [0], (ns, P, Cc, "K=1"))
        check_scan(t, chk, cands[1:3], [0, 1], (ns, P, Cc, "K=2"))
        check_scan(t, chk, cands[3:7], [0, 1, 2, 3], (ns, P, Cc, "K=4"), two_call=False)
        check_scan(t, chk, cands, [-1, 0, 18, 36], (ns, P, Cc, "K=37"))
        # ... and through the host layer: the subtree of an edge on either side, every other edge a target
        for b_sub, side in ((0, 1), (ot.ne - 1, 0), (ot.ne // 2, 1)):
            d_sub = int(ot.er[b_sub] if side == 1 else ot.el[b_sub])
            for link_is_left in (True, False):
                if not link_is_left and d_sub < ot.n:
                    continue
                targets = [e for e in range(ot.ne) if e != b_sub]
                ll = [0.3 * float(tree.edge_len[e]) + 0.001 for e in targets]
                lr = [0.7 * float(tree.edge_len[e]) + 0.002 for e in targets]
                l_sub = float(tree.edge_len[b_sub]) * 1.5
                got = t.Regraft_Scan(b_sub, d_sub, link_is_left, l_sub, targets, ll, lr)
                sub = d_sub if d_sub < ot.n else t.side_buffer(b_sub, side)
                for i, e in enumerate(targets):
                    c1 = int(ot.el[e]) if ot.el[e] < ot.n else t.side_buffer(e, 0)
                    c2 = int(ot.er[e]) if ot.er[e] < ot.n else t.side_buffer(e, 1)
                    ref = chk.candidate((c1, c2, sub, 0 if link_is_left else LEFT, ll[i], lr[i], l_sub))[0]
                    assert within_bar(got[i], ref), ("Lk_Regraft_Scan", b_sub, side, link_is_left, e, got[i], ref)
    finally:
        t.close()


# 2. rare branches: each asserted on the oracle's own output first ---------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_scaling_exponents_zero_inherited_and_own(ns):
    """A deep tree with long branches: among the kept exponent vectors are 0, sums inherited from the children, and a candidate's own
    +256 on top of what it inherited or on nothing.  (20 states: the join is recomputed in a second pass that applies 2^256 and reads
    the inherited exponents through the fragment-major layout -- other code than the 4-state registers.)"""
    t, ot, tree, st = (synthetic_pair(300, 24, 4, 4, seed=5, lmin=1.0, lmax=4.0) if ns == 4 else
                       synthetic_pair(120, 24, 20, 4, seed=5, lmin=1.0, lmax=3.0))
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        chk = Checker.of_tree(t, ot)
        w = ot.wght > 0
        total = {idx: int(sc[w].max()) for idx, (p, sc) in chk.buf.items()}
        order = sorted(total, key=lambda i: (total[i], i))
        zero = [i for i in order if total[i] == 0]
        scaled = [i for i in order if total[i] > 0]
        assert zero and scaled
        assert {int(v) for p, sc in chk.buf.values() for v in np.unique(sc[w])} == {0, 256, 512}
        rng = np.random.default_rng(2)
        pairs = [(zero[0], zero[1]), (scaled[0], zero[0]), (scaled[-1], scaled[-2])]
        pairs += [(int(rng.choice(order)), int(rng.choice(order))) for _ in range(40)]
        cands, seen = [], set()
        for (a, b) in pairs:
            c = (a, b, zero[2], 0, 2.5, 3.0, 0.4)
            ref = chk.candidate(c)
            s1, s2 = chk.buf[a][1], chk.buf[b][1]
            own = ref[3] - s1 - s2
            assert set(np.unique(own[w])) <= {0, 256}
            kinds = set()
            if np.any((ref[3] == 0)[w]): kinds.add("zero")
            if np.any(((own == 0) & (ref[3] > 0))[w]): kinds.add("inherited")
            if np.any((own == 256)[w]): kinds.add("own")
            if kinds - seen or len(cands) < 3:
                cands.append(c)
                seen |= kinds
        assert seen == {"zero", "inherited", "own"}, seen
        check_scan(t, chk, cands, list(range(len(cands))), "scaling", two_call=len(cands) <= 8)
    finally:
        t.close()


def test_all_ones_shortcut_of_fully_ambiguous_tips():
    """Tip x tip candidates whose tips are both fully ambiguous at some patterns: the oracle's vector is exactly 1.0 there."""
    n, P = SMALL_SHAPES[4]
    t, ot, tree = prepared(n, P, 4, 4)
    try:
        for tip in (1, 2):   # through the ABI's per-pattern setter, and into the oracle's tip arrays
            for p in (3, 100, 299):
                t.inst.set_tip_partials_at_pattern(tip, p, np.ones(4))
                ot.tip_vec[tip][p, :] = 1.0; ot.tip_amb[tip][p] = 1
        t.Lk(None); ot.lk(None, both_sides=True)   # (the tree's own vectors follow the tips)
        chk = Checker.of_tree(t, ot)
        both = np.all(ot.tip_vec[0] == 1.0, axis=1) & np.all(ot.tip_vec[5] == 1.0, axis=1)
        assert both.sum() >= 3   # 'N' / '-' / '?' of the synthetic alignment
        cands = [(1, 2, t.side_buffer(0, 0) if ot.el[0] >= ot.n else t.side_buffer(0, 1), 0, 0.1, 0.2, 0.3), (0, 5, 3, 0, 0.3, 0.05, 0.2),
                 (2, 1, sorted(chk.buf)[0], LEFT, 0.4, 0.1, 0.15)]
        for c, pats in ((cands[0], [3, 100, 299]), (cands[1], np.flatnonzero(both)), (cands[2], [3, 100, 299])):
            vec = chk.candidate(c)[2]
            assert np.all(vec[pats] == 1.0) and not np.all(vec == 1.0)
            # (the general product would not give 1.0: the rounded row sums of the matrices differ from it somewhere)
        rows = np.concatenate([chk.pmat(l).sum(axis=2).ravel() for l in (0.1, 0.2, 0.3, 0.05, 0.4)])
        print("row sums of the candidates' matrices that are not exactly 1.0:", int((rows != 1.0).sum()), "of", rows.size)
        check_scan(t, chk, cands, [0, 1, 2], "all-ones")
    finally:
        t.close()


@pytest.mark.parametrize("name", ["nucleic_zero_w", "nucleic_gtr_g4_inv"])
def test_zero_weight_patterns_and_invariant_sites(name, golden):
    d = golden(name)
    t, ot = device_tree_from_golden(d)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        if name == "nucleic_zero_w":
            assert np.any(ot.wght == 0) and int((ot.wght > 0).sum()) >= 300
        else:
            assert ot.m.invar_model == 1 and ot.m.pinvar > 0 and np.any(ot.invar >= 0)
        chk = Checker.of_tree(t, ot)
        cands = raw_records(t, ot, 16, seed=9)
        check_scan(t, chk, cands, [-1, 0, 7, 15], name, two_call=False)
        check_scan(t, chk, cands[:3], [0], name)
    finally:
        t.close()


def test_small_floor_raises_the_candidates_own_warning():
    """Two internal vectors rewritten so that some patterns underflow in every candidate that reads both: the SMALL floor, with the
    warning in outWarnings of those candidates only -- the instance's own flag stays 0 (tests/test_gpu_exact_site.py's recipe)."""
    n, P = SMALL_SHAPES[4]
    t, ot, tree = prepared(n, P, 4, 4)
    try:
        chk = Checker.of_tree(t, ot)
        a, b, c = sorted(chk.buf)[:3]
        for idx in (a, b):
            p, sc = chk.buf[idx]
            p = p.copy(); p[1::7] *= 1e-200
            chk.buf[idx] = (p, sc)
            t.inst.set_partials(idx, p)
        assert t.inst.numerical_warning() == 0
        cands = [(a, b, c, 0, 0.1, 0.2, 0.3), (c, sorted(chk.buf)[3], 0, 0, 0.1, 0.2, 0.3), (a, b, c, LEFT, 0.2, 0.1, 0.05), (a, 2, 4, 0, 0.1, 0.1, 0.1)]
        refs = [chk.candidate(x) for x in cands]
        assert [r[1] for r in refs] == [1, 0, 1, 0]
        assert refs[0][0] < -708.0 * (len(range(1, P, 7)) - 1)   # log(DBL_MIN) per floored pattern
        check_scan(t, chk, cands, [0, 1, 2, 3], "SMALL floor", two_call=False)
        assert t.inst.numerical_warning() == 0
    finally:
        t.close()


def test_without_lk_scaling():
    t, ot, tree, st = synthetic_pair(120, 40, 4, 4, seed=5, lmin=1.0, lmax=3.0, apply_scaling=0)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        assert ot.apply_scaling == 0
        chk = Checker.of_tree(t, ot)
        cands = raw_records(t, ot, 8, seed=4)
        refs = [chk.candidate(c) for c in cands]
        assert all(not np.any(r[3]) for r in refs)                                 # no exponent anywhere
        assert any(0.0 < r[2][r[2] > 0].min() < 2.0 ** -256 for r in refs)         # ... where scaling would have stepped in
        check_scan(t, chk, cands, [0, 3, 7], "apply_lk_scaling = 0", two_call=False)
    finally:
        t.close()


def test_without_lk_scaling_at_twenty_states():
    """the same at 20 states: the second pass of the join must not apply 2^256 and the tail's f stays 0 (the smallest positive
    partial of the tree is 2.0e-206, far below 2^-256)"""
    t, ot, tree, st = synthetic_pair(120, 24, 20, 4, seed=5, lmin=1.0, lmax=3.0, apply_scaling=0)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        assert ot.apply_scaling == 0 and not any(np.any(s) for s in ot.scale.values())
        assert min(float(p[p > 0].min()) for p in ot.plk.values()) < 1e-200
        chk = Checker.of_tree(t, ot)
        cands = raw_records(t, ot, 8, seed=4)
        refs = [chk.candidate(c) for c in cands]
        assert all(not np.any(r[3]) for r in refs)
        assert any(0.0 < r[2][r[2] > 0].min() < 2.0 ** -256 for r in refs)
        check_scan(t, chk, cands, [0, 3, 7], "apply_lk_scaling = 0, 20 states", two_call=False)
    finally:
        t.close()


def test_invariant_sites_at_twenty_states_with_scaled_constant_patterns():
    """+I at 20 states on a deep tree with planted constant columns: in most candidates some constant pattern reaches the tail with a
    nonzero exponent (the kept vector's plus the subtree's; asserted on the oracle), in some none does"""
    t, ot, tree, st = synthetic_pair(90, 24, 20, 4, seed=5, lmin=4.0, lmax=8.0, pinvar=0.2, constant_every=4)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        const = ot.invar >= 0
        assert ot.m.invar_model == 1 and ot.m.pinvar == 0.2 and 4 <= int(const.sum()) < ot.P
        chk = Checker.of_tree(t, ot)
        cands = raw_records(t, ot, 16, seed=9)
        scaled = []
        for c in cands:
            f = chk.candidate(c)[3] + (chk.buf[c[2]][1] if c[2] >= ot.n else 0)
            scaled.append(bool(np.any(f[const] != 0)))
        assert sum(scaled) >= 4 and not all(scaled), scaled
        check_scan(t, chk, cands, [-1, 0, 7, 15], "+I at 20 states", two_call=False)
        check_scan(t, chk, cands[:3], [0], "+I at 20 states")
    finally:
        t.close()


# 3. bits that must not move --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_a_candidates_bits_depend_on_the_candidate_alone(ns, small):
    t, ot, tree, cands, base = small(ns)
    assert np.array_equal(t.inst.regraft_log_likelihoods(cands), base)            # the same call twice
    for k in (0, 18, 36):                                                         # first, middle, last of 37 -- and alone
        assert t.inst.regraft_log_likelihoods([cands[k]])[0] == base[k]
    perm = np.random.default_rng(1).permutation(len(cands))
    got = t.inst.regraft_log_likelihoods([cands[i] for i in perm])
    assert all(got[j] == base[i] for j, i in enumerate(perm))
    # the work space bounded to 12 candidates: 37 run in four chunks
    P, Cc = ot.P, ot.m.ncatg
    fixed = P * Cc * ns * 8 + ((P + 1) // 2 * 2) * 4
    per = 3 * Cc * ns * ns * 8 + (P + 255) // 256 * 8 + 72
    bound = fixed + 12 * per + per // 2
    assert capi.regraft_chunk_candidates(P, Cc, ns, bound) == 12 and -(-len(cands) // 12) >= 3
    t.inst.set_regraft_work_space(bound)
    try:
        w = ot.wght > 0
        chunked = t.inst.regraft_log_likelihoods(cands, keep=5)
        assert np.array_equal(chunked, base)
        vec, sc = t.inst.regraft_partials()                                     # kept in the first chunk, read after the last
        ref = Checker.of_tree(t, ot).candidate(cands[5])
        assert np.array_equal(vec[w], ref[2][w]) and np.array_equal(sc[w], ref[3][w])
        assert np.array_equal(t.inst.regraft_transition_matrix(36, 2), ref_pm(t, ot, cands[36][6]))   # the last chunk's are there
        with pytest.raises(capi.PhyhipError) as ei:
            t.inst.regraft_transition_matrix(0, 0)                                                   # an earlier chunk's have left
        assert ei.value.code == capi.ERROR_OUT_OF_RANGE
    finally:
        t.inst.set_regraft_work_space(0)
    assert np.array_equal(t.inst.regraft_log_likelihoods(cands), base)


def ref_pm(t, ot, l):
    return Checker(ot, {}).pmat(l)


@pytest.mark.parametrize("ns", [4, 20])
def test_shards_on_one_device(ns, small):
    t1, ot, tree, cands, base = small(ns)
    chk = Checker.of_tree(t1, ot)
    refs = [chk.candidate(c) for c in cands]
    t1.inst.regraft_log_likelihoods(cands, keep=9)
    kept = t1.inst.regraft_partials()
    n, P = SMALL_SHAPES[ns]
    for shards in (1, 2, 3):
        t, _, _, _ = synthetic_pair(n, P, ns, 4, seed=SEED, ambiguous_every=5, devices=[0] * shards, force_sharded=True)
        try:
            assert len(t.inst.shard_ranges()) == shards
            t.Set_Both_Sides(True)
            t.Lk(None)
            assert all(t.side_buffer(e, s) == t1.side_buffer(e, s) for (e, s) in ot.plk)
            lnl, warn = t.inst.regraft_log_likelihoods(cands, keep=9, with_warnings=True)
            for k, r in enumerate(refs):
                assert within_bar(lnl[k], r[0]) and warn[k] == r[1], (shards, k, lnl[k], r[0])
            vec, sc = t.inst.regraft_partials()
            assert np.array_equal(vec, kept[0]) and np.array_equal(sc, kept[1])
            assert np.array_equal(t.inst.regraft_transition_matrix(36, 1), t1.inst.regraft_transition_matrix(36, 1))
            assert np.array_equal(t.inst.regraft_log_likelihoods(cands), lnl)
        finally:
            t.close()


# 4. isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_a_scan_changes_nothing_but_its_work_space(ns):
    n, P = SMALL_SHAPES[ns]
    t, ot, tree = prepared(n, P, ns, 4)
    try:
        e = next(k for k in range(ot.ne) if ot.el[k] >= ot.n and ot.er[k] >= ot.n)
        t.Update_Eigen_Lr(e)
        t.Lk(e); ot.lk(e)
        before = (t.inst.site_outputs(), t.inst.get_dot_prod(), t.inst.numerical_warning(),
                  [t.inst.get_transition_matrix(k) for k in range(ot.ne + 4)])
        cands = raw_records(t, ot, 12, seed=8)
        t.inst.regraft_log_likelihoods(cands, keep=4)
        assert_device_state_is_the_oracles(t, ot, what="after a scan")
        after = (t.inst.site_outputs(), t.inst.get_dot_prod(), t.inst.numerical_warning(),
                 [t.inst.get_transition_matrix(k) for k in range(ot.ne + 4)])
        assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
        assert np.array_equal(before[1], after[1]) and before[2] == after[2]
        assert all(np.array_equal(a, b) for a, b in zip(before[3], after[3]))
    finally:
        t.close()


def test_a_queued_path_update_is_seen():
    n, P = SMALL_SHAPES[4]
    t, ot, tree = prepared(n, P, 4, 4)
    try:
        e = next(k for k in range(ot.ne) if ot.el[k] >= ot.n and ot.er[k] >= ot.n)
        d = int(ot.el[e])
        nb = next(be for (v, be) in ot.adj[d] if be != e)   # a neighbouring edge changes length, the side of e on d follows
        ot.len[nb] = float(ot.len[nb]) * 3.0 + 0.05
        ot.update_pmat(nb); ot.update_partial(e, d)
        t.edge(nb).contents.l = float(ot.len[nb])
        t.Update_PMat_At_Given_Edge(nb)
        t.Update_Partial_Lk(e, d)                           # queued, not launched
        chk = Checker.of_tree(t, ot)
        target = t.side_buffer(e, 0)
        other = t.side_buffer(e, 1)
        cands = [(target, other, 0, 0, 0.1, 0.2, 0.3), (2, target, other, LEFT, 0.3, 0.1, 0.2)]
        check_scan(t, chk, cands, [0, 1], "queued path update", two_call=False)
        assert_device_state_is_the_oracles(t, ot, what="the queued update ran")
    finally:
        t.close()


@pytest.mark.parametrize("ns,P", [(4, 150), (20, 40)])
def test_virtual_buffers_are_stored_for_the_call(ns, P):
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
            cands = raw_records(t, ot, 24, seed=12)
            got[virtual] = t.inst.regraft_log_likelihoods(cands)
            if virtual:
                assert t.inst.virtual_stats()[0] < now and t.inst.virtual_stats()[3] > 0
            chk = Checker.of_tree(t, ot)
            assert all(within_bar(v, chk.candidate(c)[0]) for v, c in zip(got[virtual], cands))
        finally:
            t.close()
    assert np.array_equal(got[True], got[False])


def test_lk_and_dlk_after_a_scan_are_served_resident_again():
    t, ot, tree, st = synthetic_pair(14, 382, 4, 4, seed=23, ambiguous_every=17)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        e = 3
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        lkb = t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        chain = lambda: [t.dLk(0.003 * (i + 1), e) for i in range(6)]
        first = chain()
        served, _, _, instead = t.inst.resident_stats(0)
        assert served > 0
        cands = raw_records(t, ot, 20, seed=3)
        t.inst.regraft_log_likelihoods(cands, keep=2)
        again = chain()
        assert first == again
        now = t.inst.resident_stats(0)
        assert now[0] == served + len(again) and now[3] == instead, (served, instead, now)
        t.Set_Use_Eigen_Lr(False)
        t.Lk(e)
        s0 = t.inst.resident_stats(1)
        a = t.Lk(e)
        s1 = t.inst.resident_stats(1)
        t.inst.regraft_log_likelihoods(cands)
        b = t.Lk(e)
        s2 = t.inst.resident_stats(1)
        assert a == b
        print("Lk(b) served by the short-launch resident evaluator before / after the scan:", s1[0] - s0[0], s2[0] - s1[0])
        if s1[0] == s0[0] + 1:                              # where the short-launch evaluator served Lk(b), it serves it again
            assert s2[0] == s1[0] + 1 and s2[3] == s1[3], (s0, s1, s2)
    finally:
        t.close()


# 5. a real search's candidates -----------------------------------------------------------------------------------------------------
def device_tree_from_recorded(d):
    from phyml_amd import lktree
    n, P, S, Cc = int(d["n_otu"][0]), int(d["n_pattern"][0]), int(d["ns"][0]), int(d["ncatg"][0])
    t = lktree.LkTree(n, d["edge_left"], d["edge_rght"], d["edge_len"], P, S, Cc, host_pmat=True)
    t.set_model(d["pi"], d["gamma_rr"], d["gamma_r_proba"], d["e_val"], d["r_e_vect"], d["l_e_vect"], float(d["l_min"][0]),
                float(d["l_max"][0]), float(d["br_len_mult"][0]), int(d["apply_lk_scaling"][0]), int(d["invar_model"][0]),
                float(d["pinvar"][0]))
    t.Make_Tree_For_Lk(d["wght"], d["invar"])
    tv, _, _ = replay.tips_from_masks(d["tip_mask"], S)
    t.set_tips(tip_partials=tv)
    return t


@pytest.mark.parametrize("name", ["trace_nucleic_spr", "trace_proteic_spr"])
def test_candidates_of_a_recorded_search(name):
    """The recorded stream replayed in slices; in front of each of its first 40 regraft candidates (two SET_PMAT, UPDATE, SET_PMAT,
    EDGE_LNL) five variants of it are scanned: the recorded lengths, and the same target length split at 0.1, 0.25, 0.75, 0.9.
    Variant 0 against what the reference returned (1e-10: the bound tests/test_gpu_trace.py sets for device-built matrices), all five
    against the oracle that replayed the same slices."""
    d = phyg.load(os.path.join(GOLDEN, name + ".phyg"))
    tr, ref_out, _ = replay.recorded_trace(d)
    kind = tr["kind"]
    pat = [replay.SET_PMAT, replay.SET_PMAT, replay.UPDATE, replay.SET_PMAT, replay.EDGE_LNL]
    starts = [i for i in range(len(kind) - 4) if list(kind[i:i + 5]) == pat][:40]
    assert len(starts) == 40
    t = device_tree_from_recorded(d)
    ot = tree_from_recorded(d)
    rr = RecordedReplayer(ot)
    try:
        pos, last_len, worst, worst_rec = 0, {}, 0.0, 0.0
        cut = lambda a, b: {k: v[a:b] for k, v in tr.items()}
        for s in starts:
            if s > pos:
                t.Replay_Surface_Trace(cut(pos, s))
                rr.run(cut(pos, s))
            for i in range(pos, s + 5):
                if kind[i] == replay.SET_PMAT:
                    last_len[int(tr["a"][i])] = float(tr["x"][i])
            u, ev = s + 2, s + 4
            dest, c1, m1, c2, m2 = (int(tr[k][u]) for k in ("a", "b", "c", "d", "e"))
            left, rght, m3 = int(tr["a"][ev]), int(tr["b"][ev]), int(tr["c"][ev])
            assert dest in (left, rght)
            sub, flags = (rght, 0) if left == dest else (left, LEFT)
            l1, l2, l3 = last_len[m1], last_len[m2], last_len[m3]
            tot = l1 + l2
            cands = [(c1, c2, sub, flags, l1, l2, l3)] + [(c1, c2, sub, flags, f * tot, tot - f * tot, l3) for f in (0.1, 0.25, 0.75, 0.9)]
            chk = Checker(ot, {idx: v for idx, v in rr.bufs.items()})
            got = t.inst.regraft_log_likelihoods(cands)
            rec = abs(got[0] - ref_out[ev]) / abs(ref_out[ev])
            worst_rec = max(worst_rec, rec)
            assert rec < 1e-10, (name, s, got[0], ref_out[ev])
            for k, c in enumerate(cands):
                ref = chk.candidate(c)[0]
                worst = max(worst, abs(got[k] - ref) / abs(ref))
                assert within_bar(got[k], ref), (name, s, k, got[k], ref)
            out, _ = t.Replay_Surface_Trace(cut(s, s + 5))           # the candidate's own records, the existing route
            ref5, _ = rr.run(cut(s, s + 5))
            assert within_bar(out[4], ref5[4]) and got[0] == pytest.approx(out[4], rel=1e-11)
            pos = s + 5
        print(name, "worst relative difference to the oracle", worst, "to the recorded scalar", worst_rec)
    finally:
        t.close()


# 6. the error table ----------------------------------------------------------------------------------------------------------------
def _refused(fn, *a, **kw):
    with pytest.raises(capi.PhyhipError) as ei:
        fn(*a, **kw)
    return ei.value.code, str(ei.value)


def test_error_table(small):
    t, ot, tree, cands, base = small(4)
    inst = t.inst
    nbuf = max(t.side_buffer(e, s) for (e, s) in ot.plk) + 1 + 4
    good = cands[0]
    who = "phyhip_calculate_regraft_log_likelihoods"
    bad = [((-1,) + good[1:], "buffer"), ((good[0], nbuf + 50) + good[2:], "buffer"), (good[:2] + (nbuf + 50,) + good[3:], "buffer"),
           ((good[0], good[1], 0, LEFT) + good[4:], "left operand")]
    for c, _ in bad:
        code, msg = _refused(inst.regraft_log_likelihoods, [good, c])
        assert code == capi.ERROR_OUT_OF_RANGE and who in msg, msg
    for kw in (dict(keep=1), dict(keep=7), dict(keep=-2), dict(eigen_index=1), dict(eigen_index=-1)):
        code, msg = _refused(inst.regraft_log_likelihoods, [good], **kw)
        assert code == capi.ERROR_OUT_OF_RANGE and who in msg, (kw, msg)
    inst.regraft_log_likelihoods(cands)
    for which in (-1, 3):
        code, msg = _refused(inst.regraft_transition_matrix, 0, which)
        assert code == capi.ERROR_OUT_OF_RANGE and "phyhip_get_regraft_transition_matrix" in msg
    code, msg = _refused(inst.regraft_transition_matrix, len(cands), 0)
    assert code == capi.ERROR_OUT_OF_RANGE
    code, msg = _refused(inst.regraft_partials)                      # the last call kept nothing
    assert code == capi.ERROR_OUT_OF_RANGE and "phyhip_get_regraft_partials" in msg
    assert inst.regraft_log_likelihoods([]).size == 0                 # count == 0 succeeds and does nothing
    assert np.array_equal(inst.regraft_log_likelihoods(cands), base)  # ... and the instance is still usable
    # getters before any call; refusals by kind of instance
    fresh = capi.Instance(4, 10, 4, 16, 5, 4)
    try:
        for fn, a, name in ((fresh.regraft_partials, (), "phyhip_get_regraft_partials"),
                            (fresh.regraft_transition_matrix, (0, 0), "phyhip_get_regraft_transition_matrix")):
            code, msg = _refused(fn, *a)
            assert code == capi.ERROR_OUT_OF_RANGE and name in msg, msg
        assert fresh.profile_read_regraft() == (0.0, 0, 0)
    finally:
        fresh.close()
    rec = [(4, 5, 6, 0, 0.1, 0.1, 0.1)]
    # (an instance of a state count other than 4 / 20 cannot be created: phyhip_create_instance refuses it)
    for make in (lambda: capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True), lambda: capi.Instance(4, 10, 4, 16, 5, 9),
                 lambda: capi.Instance(4, 10, 20, 16, 5, 16)):
        x = make()
        try:
            code, msg = _refused(x.regraft_log_likelihoods, rec)
            assert code == capi.ERROR_NO_IMPLEMENTATION and who in msg, msg
        finally:
            x.close()
    rank = capi.Instance(4, 10, 4, 16, 5, 4)
    try:
        rank.comm_init_rank(1, 0, capi.comm_get_unique_id())
        code, msg = _refused(rank.regraft_log_likelihoods, rec)
        assert code == capi.ERROR_NO_IMPLEMENTATION and who in msg, msg
    finally:
        rank.close()
    g, _, _, _ = synthetic_pair(6, 40, 4, 4, seed=5, use_m4mod=True)   # the reference's generic loop
    try:
        g.Set_Both_Sides(True); g.Lk(None)
        code, msg = _refused(g.inst.regraft_log_likelihoods, [(0, 1, 2, 0, 0.1, 0.1, 0.1)])
        assert code == capi.ERROR_NO_IMPLEMENTATION and who in msg, msg
        assert g.Lk(None) < 0.0
    finally:
        g.close()


def test_profile_counts_calls_and_candidates(small):
    t, ot, tree, cands, base = small(20)
    t.inst.profile(1)
    try:
        t.inst.regraft_log_likelihoods(cands)
        t.inst.regraft_log_likelihoods(cands[:5])
        ms, calls, n = t.inst.profile_read_regraft()
        assert ms > 0.0 and calls == 2 and n == len(cands) + 5
        assert t.inst.profile_read_regraft() == (0.0, 0, 0)
    finally:
        t.inst.profile(0)
