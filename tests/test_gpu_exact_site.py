"""phyhip_calculate_edge_site_outputs_exact (phyml_amd/csrc/phyhip_exact.hip; Get_Exact_Site_Lk in the host layer): the per-pattern
outputs of Lk_Core -- c_lnL_sorted, cur_site_lk, unscaled_site_lk_cat, fact_sum_scale -- and their ordered sum as the REFERENCE's
doubles.  Every comparison here is np.array_equal / ==: against the reference's own dumps at the root edge of the six fixtures,
against the CPU restatement (orc_edge_lnl, arith = 1) at every edge and on synthetic shapes.  The one tolerance is the golden lnL
(1e-14 relative: the bound the restatement itself is held to).  Patterns without weight are masked as in
tests/test_oracle_golden.py (the reference skips them; the device writes zeros there)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from conftest import FIXTURES
from gpu_common import device_tree_from_golden, synthetic_oracle, synthetic_pair
from phyml_amd import capi, lktree

ARRAYS = ("c_lnL_sorted", "cur_site_lk", "unscaled_site_lk_cat", "fact_sum_scale")


def oracle_edge(P, Cc, S, wght, left, rght, pm, pi, cat_w, invar_model=0, pinvar=0.0, invar=None, apply_scaling=1):
    """orc_edge_lnl(arith = 1) on two orc.Side records: (sum, [c_lnL_sorted, cur_site_lk, unscaled_site_lk_cat, fact_sum_scale], warning)"""
    out = [np.zeros(P), np.zeros(P), np.zeros((P, Cc)), np.zeros(P, np.int32)]
    warn = C.c_int(0)
    p = orc._p
    v = orc.lib().orc_edge_lnl(C.c_int(P), C.c_int(Cc), C.c_int(S), p(orc.f64(wght)), C.byref(left), C.byref(rght), p(orc.f64(pm)),
                               p(orc.f64(pi)), p(orc.f64(cat_w)), C.c_int(invar_model), C.c_double(pinvar),
                               p(None if invar is None else np.ascontiguousarray(invar, dtype=np.int16)), C.c_int(apply_scaling), C.c_int(1),
                               p(out[0]), p(out[1]), p(out[2]), p(out[3]), C.byref(warn))
    return v, out, warn.value


def assert_edge_is_the_oracles(t, ot, e, what=None):
    """The exact route at edge e against the restatement's evaluation of that edge (partials on both sides current in both)."""
    got_sum, *got = t.Exact_Site_Lk(e)
    ref_sum = ot.lk(e, refresh_pmat=False)
    w = ot.wght > 0
    for g, k in zip(got, ARRAYS):
        assert np.array_equal(g[w], getattr(ot, k)[w]), (what, e, k)
        assert not np.any(g[~w]), (what, e, k, "patterns without weight are written as 0")
    assert got_sum == ref_sum, (what, e, got_sum, ref_sum)


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
            cache[name] = (d, t, ot, ot.lk(None, both_sides=True))
        return cache[name]
    yield get
    for v in cache.values():
        v[1].close()


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_root_edge_is_the_references_dump(name, evaluated):
    d, t, ot, ot_lnl = evaluated(name)
    got_sum, *got = t.Exact_Site_Lk(None)
    w = d["wght"] > 0
    assert int(w.sum()) >= 300 if name == "nucleic_zero_w" else bool(w.all())
    for g, k in zip(got, ARRAYS):
        assert np.array_equal(g[w], d[k][w]), (name, k)
    assert got_sum == ot_lnl
    assert abs(got_sum - d["lnL"][0]) <= 1e-14 * abs(d["lnL"][0])
    # the host layer asked for the edge Lk(NULL) evaluates; the C ABI addressed directly says the same
    b = t.edge(ot.root_edge()).contents
    child = b.p_lk_tip_idx if b.rght.contents.tax else b.p_lk_rght_idx
    a, c, u, f, s, warn = t.inst.exact_site_outputs(b.p_lk_left_idx, child, b.Pij_rr_idx)
    assert s == got_sum and warn == 0
    for g, h in zip(got, (a, c, u, f)):
        assert np.array_equal(g, h)


# 2, 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_every_edge_is_the_oracles(name, evaluated):
    d, t, ot, _ = evaluated(name)
    for e in range(t.ne):
        assert_edge_is_the_oracles(t, ot, e, name)


def test_the_fixtures_reach_every_branch(evaluated):
    """Nothing silently absent: each case of the route is counted over the edges test_every_edge_is_the_oracles walks."""
    n = dict(onehot=0, ambiguous=0, internal=0, scaled=0, invariant=0)
    for name in FIXTURES:
        d, t, ot, _ = evaluated(name)
        w = ot.wght > 0
        for e in range(ot.ne):
            r = int(ot.er[e])
            if r < ot.n:
                n["onehot"] += int((w & (ot.tip_amb[r] == 0)).sum())      # right tip, one state: the tip branch
                n["ambiguous"] += int((w & (ot.tip_amb[r] != 0)).sum())   # right tip, several states: the general branch on a tip
            else:
                n["internal"] += int(w.sum())
            if name in ("synth_nt_300x40", "synth_aa_90x24") and e % 16 == 0:
                ot.lk(e, refresh_pmat=False)
                n["scaled"] += int((w & (ot.fact_sum_scale != 0)).sum())
        if ot.m.invar_model:
            n["invariant"] += int((w & (ot.invar >= 0)).sum())
    print(n)
    assert all(v > 0 for v in n.values()), n


# 4 ------------------------------------------------------------------------------------------------------------------------
ROUTES = [(1, True), (0, False), (1, False), (0, True)]  # (apply_scaling, host_pmat)


@pytest.mark.parametrize("ns", [4, 20])
@pytest.mark.parametrize("Cc", [1, 3, 4, 8, 9, 64])
def test_synthetic_shapes(ns, Cc):
    """Every category count (one to 64: all three device layouts, more categories than a wave-tile holds) at every pattern
    count around the wave and workgroup sizes, weights with zeros; scaling on / off and both matrix routes rotate over the
    pattern counts so that each (states, categories) sees all four combinations and each pattern count sees them over the
    category counts.  Every edge of a 6-taxon tree: tips on the right (one state, several states), internal on the right."""
    for i, P in enumerate([1, 63, 64, 65, 257]):
        scaling, host_pmat = ROUTES[(i + Cc) % 4]
        wght = np.array([0.0 if (k % 5 == 3) else 1.0 + (k % 3) for k in range(P)])
        t, ot, tree, st = synthetic_pair(6, P, ns, Cc, seed=100 + P + Cc, wght=wght, apply_scaling=scaling, host_pmat=host_pmat,
                                         ambiguous_every=4)
        try:
            t.Set_Both_Sides(True)
            t.Lk(None)
            ot.lk(None, both_sides=True)
            for e in range(t.ne):
                assert_edge_is_the_oracles(t, ot, e, (ns, Cc, P, scaling, host_pmat))
        finally:
            t.close()


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nucleic_gtr_g4", "proteic_lg_g4"])
def test_a_left_hand_tip(name, evaluated):
    """Through the C ABI directly: the parent index a tip, the child an internal buffer -- the edge turned round.  The left tip
    enters as its 0/1 vector in every category and the right side, being no tip, takes the general branch."""
    d, t, ot, _ = evaluated(name)
    m = ot.m
    w = ot.wght > 0
    edges = [e for e in range(ot.ne) if ot.er[e] < ot.n and ot.el[e] >= ot.n][:3]
    assert edges
    for e in edges:
        tip = int(ot.er[e])
        ref_sum, ref, _ = oracle_edge(ot.P, m.ncatg, m.ns, ot.wght, ot._side(e, 1), ot._side(e, 0), ot.pm[e], m.pi, m.gamma_r_proba,
                                      m.invar_model, m.pinvar, ot.invar, ot.apply_scaling)
        *got, got_sum, warn = t.inst.exact_site_outputs(tip, t.side_buffer(e, 0), t.edge(e).contents.Pij_rr_idx)
        for g, r in zip(got, ref):
            assert np.array_equal(g[w], r[w]), (name, e)
        assert got_sum == ref_sum and warn == 0


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_B_and_Z_are_single_states_through_the_host_layers_encoder():
    """20 states, tips set as CHARACTERS through the host layer's encoder: B and Z are the single states N and Q (src/lk.c:150-151),
    so such a tip on the right takes the tip branch -- as in the restatement built from orc.init_tip of the same characters."""
    from phyml_amd import synth
    n, P, Cc = 6, 67, 4
    ot0, tree, st, _, wg = synthetic_oracle(n, P, 20, Cc, seed=5)
    chars = synth.states_to_chars(st, 20).copy()
    for k in range(n):
        chars[k, (k * 3) % 5::5] = np.frombuffer(b"BZX-?", dtype=np.uint8)[(np.arange((k * 3) % 5, P, 5) + k) % 5]
    tv, ds, amb = zip(*[orc.init_tip(1, chars[k]) for k in range(n)])
    m = ot0.m
    ot = orc.OracleTree(m, n, tree.edge_left, tree.edge_rght, tree.edge_len, wg, tv, ds, amb)
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, 20, Cc, host_pmat=True)
    try:
        t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)
        t.Make_Tree_For_Lk(wg)
        t.set_tips(tip_chars=chars)
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        n_bz = 0
        for e in range(t.ne):
            assert_edge_is_the_oracles(t, ot, e)
            r = int(ot.er[e])
            if r < n:
                bz = (chars[r] == ord("B")) | (chars[r] == ord("Z"))
                assert not np.any(ot.tip_amb[r][bz])
                n_bz += int(bz.sum())
        assert n_bz > 0
    finally:
        t.close()


# the SMALL floor and Invariant_Lk's overflow branch: no fixture reaches them, these buffers do -------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_small_floor_and_invariant_overflow(ns):
    """Buffers set through the C ABI: a pattern whose likelihood underflows (the SMALL floor, the warning), +I patterns whose
    scaled invariant likelihood overflows (fact_sum_scale reset to 0, site_lk = pi x pinvar) and ones where it does not."""
    P, Cc = 70, 3
    rng = np.random.default_rng(7 + ns)
    left, rght = rng.uniform(0.05, 1.0, (P, Cc * ns)), rng.uniform(0.05, 1.0, (P, Cc * ns))
    sl, sr = np.zeros(P, np.int32), np.zeros(P, np.int32)
    invar = np.full(P, -1, np.int16)
    left[1::7] *= 1e-200; rght[1::7] *= 1e-200         # underflow: the floor
    invar[2::7] = (np.arange(2, P, 7) % ns); sl[2::7] = 768; sr[2::7] = 512   # pi * 2^1280 overflows
    invar[3::7] = (np.arange(3, P, 7) % ns); sl[3::7] = 256                    # scaled, finite
    invar[4::7] = (np.arange(4, P, 7) % ns)                                    # unscaled +I
    sr[5::7] = 256                                                            # scaled, not invariant
    wght = np.array([0.0 if k % 11 == 6 else 1.0 + k % 2 for k in range(P)])
    pm = rng.uniform(0.01, 1.0, (Cc, ns, ns)); pm /= pm.sum(axis=2, keepdims=True)
    pi = rng.uniform(0.5, 1.0, ns); pi /= pi.sum()
    cw = np.array([0.2, 0.5, 0.3])
    pinvar = 0.23
    inst = capi.Instance(2, 4, ns, P, 1, Cc)
    try:
        inst.set_phyml_options(apply_lk_scaling=1)
        inst.set_pattern_weights(wght); inst.set_category_weights(cw); inst.set_state_frequencies(pi)
        inst.set_invariant_sites(1, pinvar, invar)
        inst.set_transition_matrix(0, pm)
        inst.set_partials(2, left); inst.set_partials(3, rght)
        for b, s in ((2, sl), (3, sr)):
            capi._chk(inst.L.phyhip_set_scale_factors(inst.id, b, capi._ptr(s)))
        a = orc.Side(); a.p_lk = orc._p(left); a.sum_scale = orc._p(sl); a.is_tip = 0
        b = orc.Side(); b.p_lk = orc._p(rght); b.sum_scale = orc._p(sr); b.is_tip = 0
        ref_sum, ref, ref_warn = oracle_edge(P, Cc, ns, wght, a, b, pm, pi, cw, 1, pinvar, invar, 1)
        *got, got_sum, warn = inst.exact_site_outputs(2, 3, 0)
        w = wght > 0
        for g, r in zip(got, ref):
            assert np.array_equal(g[w], r[w])
        assert got_sum == ref_sum and warn == ref_warn == 1
        # the branches were taken: the floor's value, and the overflow's reset of the scaling exponent
        assert np.all(got[0][1::7][w[1::7]] < -708.0) and np.all(got[0][0::7][w[0::7]] > -700.0)   # log(DBL_MIN) = -708.39...
        assert np.all(got[3][2::7] == 0) and np.all(got[3][3::7][w[3::7]] == 256)
    finally:
        inst.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nucleic_gtr_g4_inv", "proteic_lg_g4"])
def test_no_side_effects(name, golden):
    """What the hot path left and what it returns next are the same doubles with and without an exact call in between."""
    d = golden(name)
    seen = []
    for with_call in (False, True):
        t, ot = device_tree_from_golden(d)
        try:
            t.Set_Both_Sides(True)
            lnl = t.Lk(None)
            t.Lk(5)
            if with_call:
                t.Exact_Site_Lk(9)
                t.Exact_Site_Lk(None)
            out = t.inst.site_outputs()
            warn = t.inst.numerical_warning()
            if with_call:
                t.Exact_Site_Lk(2)
            seen.append((lnl, out, warn, t.Lk(7), t.Lk(None), t.partials(7, 0) if ot.el[7] >= ot.n else None))
        finally:
            t.close()
    (l0, o0, w0, a0, b0, p0), (l1, o1, w1, a1, b1, p1) = seen
    assert l0 == l1 and w0 == w1 and a0 == a1 and b0 == b1
    for x, y in zip(o0, o1):
        assert np.array_equal(x, y)
    assert (p0 is None and p1 is None) or np.array_equal(p0, p1)


@pytest.mark.parametrize("ns,P", [(4, 150), (20, 40)])
def test_a_virtual_buffer_is_stored_for_the_call(ns, P):
    """A whole-tree Lk(NULL) of more than 16 operations leaves its tip x tip results virtual; the exact route at an edge
    whose partial buffer is one of them makes it real first and returns the restatement's arrays."""
    t, ot, tree, st = synthetic_pair(26, P, ns, 4, seed=6, host_pmat=True, ambiguous_every=6)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        now, _, _, stored = t.inst.virtual_stats()
        assert now > 0 and stored == 0
        cherries = [(e, side) for (e, side) in ot.plk
                    if all(v < ot.n for (v, be) in ot.adj[int(ot.el[e] if side == 0 else ot.er[e])] if be != e)]
        assert cherries
        assert len(cherries) >= 3
        for (e, side) in cherries[:3]:   # (at most one of them is the evaluation's own and was stored)
            assert_edge_is_the_oracles(t, ot, e)
        after = t.inst.virtual_stats()
        assert after[0] < now and after[3] > 0
        for e in range(t.ne):
            assert_edge_is_the_oracles(t, ot, e)
    finally:
        t.close()


def test_resident_evaluators_still_serve_the_next_short_calls(monkeypatch):
    monkeypatch.setenv("PHYHIP_RESIDENT", "1")
    t, ot, tree, st = synthetic_pair(14, 300, 4, 4, seed=23, ambiguous_every=17)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        served = []
        for rnd in range(3):
            for e in range(t.ne):
                assert abs(t.Lk(e) - ot.lk(e, refresh_pmat=False)) <= 1e-12 * abs(ot.lk(e, refresh_pmat=False))
            served.append(t.inst.resident_stats(0)[0] + t.inst.resident_stats(1)[0])
            assert_edge_is_the_oracles(t, ot, rnd)
        assert served[0] > 0 and served[0] < served[1] < served[2], served
    finally:
        t.close()


# 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nucleic_zero_w", "synth_aa_90x24"])
def test_sharded_group_returns_the_unsharded_doubles(name, golden, evaluated):
    d, t1, ot, _ = evaluated(name)
    t, _ = device_tree_from_golden(d, devices=[0, 0, 0], force_sharded=True)
    try:
        assert len(t.inst.shard_ranges()) == 3
        t.Set_Both_Sides(True)
        t.Lk(None)
        for e in [None] + list(range(0, t.ne, max(1, t.ne // 12))):
            got, ref = t.Exact_Site_Lk(e), t1.Exact_Site_Lk(e)
            assert got[0] == ref[0], (name, e)
            for g, r in zip(got[1:], ref[1:]):
                assert np.array_equal(g, r), (name, e)
        assert_edge_is_the_oracles(t, ot, 3, name)
    finally:
        t.close()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_class_axis_and_generic_loop_instances_are_refused(golden):
    inst = capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True)
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            inst.exact_site_outputs(4, 5, 0)
    finally:
        inst.close()
    t, ot = device_tree_from_golden(golden("nucleic_gtr_g4"), use_m4mod=True, arith=2)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        b = t.edge(ot.root_edge()).contents
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            t.inst.exact_site_outputs(b.p_lk_left_idx, b.p_lk_tip_idx if b.rght.contents.tax else b.p_lk_rght_idx, b.Pij_rr_idx)
        with pytest.raises(capi.PhyhipError, match="generic-loop"):
            t.Exact_Site_Lk(None)
    finally:
        t.close()
