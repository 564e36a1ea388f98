"""Br_Len_Opt on the device (phyhip_optimise_edge_length, phyml_amd/csrc/phyhip_brlen.hip) against the real reference's records
(tests/golden/brlen_<case>.npz, tests/golden/make_brlen.py), against the host-driven chain of launched dLk calls on the same
library, and against tests/brlen_ref.py over the CPU oracle.

Bounds.  B_lnl / B_dlnl = P * 2^-52 * sum |terms| over the per-pattern lnL / dlnL terms -- the summation bound the SH tests use --
is what two orders of adding the same terms can differ by; the fixtures carry the largest over each record's probes, the synthetic
cases form it from OracleTree.dlk_terms at the result.  The evaluation count and the status are exact everywhere.  l_out is exact
(the reference's bits) where the path's best_l is the start itself or a length of one of the two walks in factors of 1.2; where it
is the spline's root it lies within eight times the spread of that root when fu, fv move by +-B_lnl and dfu, dfv by +-B_dlnl
(brlen_ref.root_spread; the fixtures carry it).  c_lnL lies within B_lnl of phyhip_calculate_eigen_lnl_dlnl at l_out (the start
itself: it is the caller's Lk(b), to the bits).  c_dlnL is the LAST probe's: on every route and at every record it is held to that
entry point evaluated at the last probe's length (brlen_ref's probes[-1] over the CPU oracle) within B_dlnl -- plus, where the last
probe is the spline's root, whose length the routes reach from their own sums, the slope of dlnL over the bracket,
|dfu - dfv| / (v - u), times twice the eight spreads the root is allowed -- and the two routes to each other within twice that."""
import os

import numpy as np
import pytest

import brlen_ref
import orc  # noqa: F401  (checker)
import phyg
from gpu_common import assert_device_state_is_the_oracles, device_tree_from_golden, synthetic_pair
from phyml_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("nucleic_gtr_g4", "nucleic_gtr_g4_inv", "proteic_lg_g4")
SPLINE_BEST = 2


def _golden(name):
    return phyg.load(os.path.join(ROOT, "tests", "golden", name + ".phyg"))


def _restore(t, e, l0):
    t.edge(e).contents.l = float(l0)
    t.Update_PMat_At_Given_Edge(e)


def _search(t, e, l_in, l0, chain=False, last_l=None):
    """(lk_begin of the device, Br_Len_Opt's tuple, whether the search ran on the device, eigen_lnl_dlnl at l_out on the edge's products,
    ... and at last_l, the numerical warning)"""
    t.edge(e).contents.l = float(l_in)
    lkb = t.Lk(e)
    r = t.Br_Len_Opt(e, force_host_chain=chain, force_device=not chain)
    dev = t.on_device
    warn = t.inst.numerical_warning()
    at = t.inst.eigen_lnl_dlnl(r[0])
    at_last = t.inst.eigen_lnl_dlnl(last_l) if last_l is not None else None
    _restore(t, e, l0)
    return lkb, r, dev, at, at_last, warn


def _oracle_replay(ot, e, l_in, l0, f=None):
    """brlen_ref over the CPU oracle on edge e from l_in (the edge restored afterwards)"""
    ot.len[e] = l_in
    lkb = ot.lk(e)
    ot.update_eigen_lr(e)
    if f is None:
        r = brlen_ref.br_len_spline(ot.dlk, l_in, lkb, ot.m.l_min, ot.m.l_max)
    else:
        r = brlen_ref.br_len_spline(ot.dlk, l_in, lkb, float(f["l_min"][0]), float(f["l_max"][0]), int(f["iter_max"][0]), float(f["tol"][0]))
    ot.len[e] = l0
    ot.update_pmat(e)
    return r


def _dlnl_bound(r, b_dlnl, spread):
    """what c_dlnL may differ by from the entry point at the oracle's last probe: the summation bound, and -- the last probe being the
    spline's root -- the slope of dlnL over the bracket times twice the eight spreads of that root"""
    if r.spline is None or r.status in (1, 2):
        return b_dlnl
    u, v, fu, fv, dfu, dfv, which, root = r.spline
    return b_dlnl + 2.0 * 8.0 * spread * abs(dfu - dfv) / (v - u)


def _near(a, b, bound):
    return a == b or abs(a - b) <= bound


@pytest.fixture(scope="module", params=CASES)
def records(request):
    """every record of a fixture through both routes, once"""
    name = request.param
    f = np.load(os.path.join(ROOT, "tests", "golden", "brlen_" + name + ".npz"))
    d = _golden(name)
    t, ot = device_tree_from_golden(d)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        dev, chain, ref = [], [], []
        for i in range(len(f["edge"])):
            e, l_in, l0 = int(f["edge"][i]), float(f["l_in"][i]), float(d["edge_len"][int(f["edge"][i])])
            ref.append(_oracle_replay(ot, e, l_in, l0, f))
            dev.append(_search(t, e, l_in, l0, last_l=ref[-1].probes[-1][0]))
            chain.append(_search(t, e, l_in, l0, chain=True, last_l=ref[-1].probes[-1][0]))
        again = [_search(t, int(f["edge"][i]), float(f["l_in"][i]), float(d["edge_len"][int(f["edge"][i])])) for i in range(0, len(f["edge"]), 7)]
    finally:
        t.close()
    return name, f, dev, chain, again, ref


def _check_route(name, f, got, ref):
    for i, (lkb, r, dev, at, at_last, warn) in enumerate(got):
        l, lnl, dlnl, ev, st = r
        b_lnl, b_dlnl, spread, bf = float(f["b_lnl"][i]), float(f["b_dlnl"][i]), float(f["root_spread"][i]), int(f["best_from"][i])
        assert ev == int(f["evaluations"][i]) and st == int(f["status"][i]), (name, i, ev, st)
        if bf != SPLINE_BEST:
            assert l == float(f["l_out"][i]), (name, i, l.hex(), float(f["l_out"][i]).hex())
        else:
            assert abs(l - float(f["l_out"][i])) <= 8.0 * spread, (name, i, l, float(f["l_out"][i]), spread)
        if bf == 0:
            assert lnl == lkb, (name, i)            # best_lnL never left the caller's c_lnL
        else:
            assert abs(lnl - at[1]) <= b_lnl, (name, i, lnl, at[1], b_lnl)
        assert warn == 0, (name, i)
        assert ref[i].evaluations == ev and ref[i].status == st, (name, i)
        bound = _dlnl_bound(ref[i], b_dlnl, spread)
        assert _near(dlnl, at_last[2], bound), (name, i, dlnl, at_last[2], bound)


def test_against_the_reference(records):
    name, f, dev, chain, again, ref = records
    assert all(d[2] for d in dev)                   # the search was the device call
    _check_route(name, f, dev, ref)


def test_against_the_host_driven_chain(records):
    name, f, dev, chain, again, ref = records
    assert not any(c[2] for c in chain)
    _check_route(name, f, chain, ref)
    for i, (a, b) in enumerate(zip(dev, chain)):
        assert a[1][3:] == b[1][3:], (name, i)      # counts and statuses
        bf, b_lnl, b_dlnl = int(f["best_from"][i]), float(f["b_lnl"][i]), float(f["b_dlnl"][i])
        if bf != SPLINE_BEST:
            assert a[1][0] == b[1][0], (name, i)
        else:
            assert abs(a[1][0] - b[1][0]) <= 8.0 * float(f["root_spread"][i]), (name, i)
        assert abs(a[1][1] - b[1][1]) <= 2.0 * b_lnl, (name, i, a[1][1], b[1][1])
        bound = 2.0 * _dlnl_bound(ref[i], b_dlnl, float(f["root_spread"][i]))
        assert _near(a[1][2], b[1][2], bound), (name, i, a[1][2], b[1][2], bound)
    for k, i in enumerate(range(0, len(dev), 7)):   # the device call repeated: the same bits
        assert again[k][1] == dev[i][1], (name, i)


# ---- geometry: W = workgroup threads, R = rounds kept in registers ---------------------------------------------------------------
def _geometry():
    out = []
    for ns in (4, 20):
        w, r = capi.BRLEN_THREADS[ns], capi.BRLEN_KEEP[ns]
        for c in (1, 3, 4, 8):
            cp = 1 << (c - 1).bit_length()
            for p in sorted({1, w // cp - 1, w // cp, w // cp + 1, r * w // cp + 1}):
                out.append((ns, c, p))
    return out


def _oracle_search(ot, e, l_in):
    l0 = float(ot.len[e])
    ot.len[e] = l_in
    lkb = ot.lk(e)
    ot.update_eigen_lr(e)
    r = brlen_ref.br_len_spline(ot.dlk, l_in, lkb, ot.m.l_min, ot.m.l_max)
    _, a, b = ot.dlk_terms(r.l)
    bounds = (ot.P * 2.0 ** -52 * float(np.abs(a).sum()), ot.P * 2.0 ** -52 * float(np.abs(b).sum()))
    b_lnl = b_dlnl = 0.0
    for (lc, _, _) in (r.probes if ot.P <= 64 else r.probes[-2:]):
        _, a, b = ot.dlk_terms(lc)
        b_lnl = max(b_lnl, ot.P * 2.0 ** -52 * float(np.abs(a).sum()))
        b_dlnl = max(b_dlnl, ot.P * 2.0 ** -52 * float(np.abs(b).sum()))
    ot.len[e] = l0
    ot.update_pmat(e)
    return r, max(bounds[0], b_lnl), max(bounds[1], b_dlnl)


def _check_synthetic(t, ot, edges, factors, what):
    t.Set_Both_Sides(True)
    t.Lk(None)
    ot.lk(None, both_sides=True)
    for e in edges:
        l0 = float(ot.len[e])
        for fct in factors:
            l_in = min(l0 * fct, 90.0)
            r, b_lnl, b_dlnl = _oracle_search(ot, e, l_in)
            last_l = r.probes[-1][0]
            lkb, d, on_dev, at, at_last, _ = _search(t, e, l_in, l0, last_l=last_l)
            _, c, on_dev_c, _, at_last_c, _ = _search(t, e, l_in, l0, chain=True, last_l=last_l)
            assert on_dev and not on_dev_c, what
            assert d[3:] == c[3:] == (r.evaluations, r.status), (what, e, fct, d, c, r.evaluations, r.status)
            if r.best_from != "spline":
                assert d[0] == c[0] == r.l, (what, e, fct)
            else:
                spread = brlen_ref.root_spread(r.spline, b_lnl, b_dlnl)
                assert abs(d[0] - r.l) <= 8.0 * spread and abs(c[0] - r.l) <= 8.0 * spread, (what, e, fct, d[0], c[0], r.l, spread)
            if r.best_from == "start":
                assert d[1] == lkb == c[1], (what, e, fct)
            else:
                assert abs(d[1] - at[1]) <= b_lnl and abs(d[1] - c[1]) <= 2.0 * b_lnl, (what, e, fct, d[1], at[1], c[1], b_lnl)
            spread = brlen_ref.root_spread(r.spline, b_lnl, b_dlnl) if r.spline is not None else 0.0
            bound = _dlnl_bound(r, b_dlnl, spread)
            assert _near(d[2], at_last[2], bound) and _near(c[2], at_last_c[2], bound), (what, e, fct, d[2], c[2], at_last[2], bound)
            assert _near(d[2], r.dlnL, 2.0 * bound) and _near(d[2], c[2], 2.0 * bound), (what, e, fct, d[2], c[2], r.dlnL, bound)


@pytest.mark.parametrize("ns,c,p", _geometry())
def test_geometry(ns, c, p):
    t, ot, tree, st = synthetic_pair(6, p, ns, c, seed=100 + p % 17 + c)
    try:
        _check_synthetic(t, ot, (0, 5), (1.0, 0.05, 20.0), (ns, c, p))
    finally:
        t.close()


# ---- the tail's branches inside the loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,edges", [("nucleic_zero_w", (0, 11, 52)), ("synth_nt_300x40", (3, 150, 400)), ("synth_aa_90x24", (3, 88, 170))])
def test_zero_weights_and_scale_exponents(name, edges):
    """bootstrap-like zero-weight patterns, and a deep tree whose edge evaluations carry nonzero scale exponents (at 20 states on
    every one of the chosen edges: the probes read them from the edge's `fact`)"""
    d = _golden(name)
    t, ot = device_tree_from_golden(d)
    try:
        _check_synthetic(t, ot, edges, (1.0, 0.05, 20.0), name)
        if name == "synth_nt_300x40":
            assert np.any(ot.fact_sum_scale != 0)
        if name == "synth_aa_90x24":
            for e in edges:
                ot.lk(e)
                assert np.any(ot.fact_sum_scale != 0), e
    finally:
        t.close()


@pytest.mark.parametrize("ns", [4, 20])
def test_the_documented_maximum_of_patterns(ns):
    """capi.BRLEN_MAX_PATTERNS patterns, 8 categories: one search at scale 1.0 on both routes"""
    assert capi.BRLEN_MAX_PATTERNS == 16384
    t, ot, tree, st = synthetic_pair(6, 16384, ns, 8, seed=3)
    try:
        _check_synthetic(t, ot, (2,), (1.0,), ("maximum", ns))
    finally:
        t.close()


# ---- the designed patterns of the tail: the SMALL floor and its warning, +I with Invariant_Lk's overflow branch -----------------------
def _designed_search(inst, E, fact, l_in, lkb):
    """the device call, the chain driven here through phyhip_calculate_eigen_lnl_dlnl, and brlen_ref over the CPU oracle on the
    device's own products: (device tuple, its warning, chain Result, its warning, oracle Result)"""
    import eigen_terms as et
    m = E.m
    dot = inst.get_dot_prod()
    dev = inst.optimise_edge_length(l_in, lkb)
    warn_dev = inst.numerical_warning()
    ch = brlen_ref.br_len_spline(inst.eigen_lnl_dlnl, l_in, lkb, m.l_min, m.l_max)
    warn_ch = inst.numerical_warning()
    ref = brlen_ref.br_len_spline(lambda l: et.oracle_sums(E, l, E.wght, dot, fact)[:3], l_in, lkb, m.l_min, m.l_max)
    return dev, warn_dev, ch, warn_ch, ref


@pytest.mark.parametrize("S,Cc", [(4, 4), (4, 3), (20, 4), (20, 1)])
@pytest.mark.parametrize("invar_late", [False, True])
def test_floored_patterns_raise_the_warning_and_the_overflow_branch(S, Cc, invar_late):
    """eigen_terms.make_edge's 70 patterns of every class: patterns floored at SMALL (the warning comes back set, from the flag in
    LDS to phyhip_get_numerical_warning), subnormal products, +I patterns scaled and unscaled, zero weights.  invar_late: the edge is
    evaluated WITHOUT the invariant model, which leaves the overflowing +I patterns' exponents at 1280, and the model is switched on
    in front of the search -- the one way to Invariant_Lk's overflow branch inside dlk_lane (tests/test_gpu_eigen_terms.py: no call
    sequence of the reference reaches it): lnL is then +inf at every probe, on every route alike."""
    import eigen_terms as et
    import test_gpu_eigen_terms as tg
    E = tg._edge(S, Cc, 70)
    inst = tg.device_edge(E)
    try:
        if invar_late:
            inst.set_invariant_sites(0, 0.0, E.invar)
        lkb = inst.edge_lnl(2, 3, 0)
        fact = inst.site_outputs()[3]
        if invar_late:
            assert np.all(fact[E.cls == et.INV_OVERFLOW] == 1280)
            inst.set_invariant_sites(E.m.invar_model, E.m.pinvar, E.invar)
        else:
            assert np.all(fact[E.cls == et.INV_OVERFLOW] == 0)
        inst.update_eigen_lr(2, 3)
        for l_in in (et.L0, et.L0 / 50.0, et.L0 * 30.0):
            dev, warn_dev, ch, warn_ch, ref = _designed_search(inst, E, fact, l_in, lkb)
            what = (S, Cc, invar_late, l_in, dev, ch[:5], ref[:5])
            assert warn_dev == 1 and warn_ch == 1, what                      # floored patterns carry weight: every probe raises it
            assert dev[3:] == (ch.evaluations, ch.status), what
            if invar_late:                                                   # (held route against route: both run dlk_lane's branch)
                assert np.isinf(ch.probes[0][1]) and ch.probes[0][1] > 0.0, what
                assert dev[1] == ch.lnL or (dev[1] != dev[1] and ch.lnL != ch.lnL), what
                assert dev[0] == ch.l or (dev[0] != dev[0] and ch.l != ch.l), what
                continue
            assert dev[3:] == (ref.evaluations, ref.status), what
            _, a, b = orc.dlk_terms(ref.l, S, Cc, E.wght, inst.get_dot_prod(), E.m, E.invar, fact, E.apply_scaling)
            b_lnl, b_dlnl = E.P * 2.0 ** -52 * float(np.abs(a).sum()), E.P * 2.0 ** -52 * float(np.abs(b).sum())
            _, a, b = orc.dlk_terms(ref.probes[-1][0], S, Cc, E.wght, inst.get_dot_prod(), E.m, E.invar, fact, E.apply_scaling)
            b_lnl = max(b_lnl, E.P * 2.0 ** -52 * float(np.abs(a).sum()))
            b_dlnl = max(b_dlnl, E.P * 2.0 ** -52 * float(np.abs(b).sum()))
            spread = brlen_ref.root_spread(ref.spline, b_lnl, b_dlnl) if ref.spline is not None else 0.0
            if ref.best_from != "spline":
                assert dev[0] == ch.l == ref.l, what
            else:
                assert abs(dev[0] - ref.l) <= 8.0 * spread and abs(ch.l - ref.l) <= 8.0 * spread, what
            if ref.best_from == "start":
                assert dev[1] == lkb
            else:
                assert _near(dev[1], inst.eigen_lnl_dlnl(dev[0])[1], b_lnl) and _near(dev[1], ch.lnL, 2.0 * b_lnl), what
            bound = _dlnl_bound(ref, b_dlnl, spread)
            assert _near(dev[2], inst.eigen_lnl_dlnl(ref.probes[-1][0])[2], bound) and _near(dev[2], ch.dlnL, 2.0 * bound), (what, bound)
        # ... and without a floored pattern under weight the flag comes back clear
        w = E.wght.copy()
        w[(E.cls == et.FLOOR) | (E.cls == et.SUBNORMAL)] = 0.0
        inst.set_pattern_weights(w)
        lkb = inst.edge_lnl(2, 3, 0)
        inst.update_eigen_lr(2, 3)
        if not invar_late:
            inst.optimise_edge_length(et.L0, lkb)
            assert inst.numerical_warning() == 0
    finally:
        inst.close()


def test_between_resident_served_evaluations():
    """A chain of dLk calls served by the resident workgroups, the device search, the chain again (the construction of
    tests/test_gpu_side_calls.py::test_parsimony_between_resident_served_evaluations): the same doubles, and every one of them served
    resident again, none launched instead -- the call is a plain one (the stream is declared dirty on entry), it waits for the stream
    and leaves it clean."""
    t, ot, tree, st = synthetic_pair(14, 382, 4, 4, seed=23, ambiguous_every=17)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        e = 3
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        lkb = t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        chain = lambda: [t.dLk(0.003 * (i + 1), e)[1] for i in range(6)]
        first = chain()
        served, _, _, instead = t.inst.resident_stats(0)
        assert served > 0
        got = t.inst.optimise_edge_length(float(tree.edge_len[e]) * 20.0, lkb)
        assert got[4] in (0, 1, 2) and got[3] >= 2
        again = chain()
        assert first == again
        now = t.inst.resident_stats(0)
        assert now[0] == served + len(again) and now[3] == instead, (served, instead, now)
        t.Set_Use_Eigen_Lr(False)
    finally:
        t.close()


# ---- the rare exits ------------------------------------------------------------------------------------------------------------
def test_upper_walk_leaves_l_max_iter_max_and_nan():
    d = _golden("nucleic_gtr_g4")
    t, ot = device_tree_from_golden(d)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        e = int(np.argmax(d["edge_len"]))
        l0 = float(d["edge_len"][e])
        # l_max below the edge's optimum: the upper walk leaves [l_min, l_max] -- status 2
        l_max = l0 / 4.0
        t.mod.contents.l_max = l_max
        t.inst.set_phyml_options(ot.m.l_min, l_max, ot.m.br_len_mult, int(d["apply_lk_scaling"][0]))
        ot.m.l_max = l_max
        try:
            l_in = l0 / 16.0
            r, _, _ = _oracle_search(ot, e, l_in)
            dv, on_dev = _search(t, e, l_in, l0)[1:3]
            ch = _search(t, e, l_in, l0, chain=True)[1]
            assert on_dev and r.status == 2
            assert dv[3:] == ch[3:] == (r.evaluations, 2) and dv[0] == ch[0] == r.l
        finally:
            ot.m.l_max = 100.0
            t.mod.contents.l_max = 100.0
            t.inst.set_phyml_options(ot.m.l_min, 100.0, ot.m.br_len_mult, int(d["apply_lk_scaling"][0]))
        _restore(t, e, l0)
        # iterMax = 1: the spline step is the first and last iteration -- status 5; the host layer stops with the reference's words
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        lkb = t.Lk(e)
        t.Set_Update_Eigen_Lr(False)
        l, lnl, dlnl, ev, st = t.inst.optimise_edge_length(l0 * 20.0, lkb, iter_max=1)
        assert st == 5 and ev >= 3
        t.s_opt.brent_it_max = 1
        with pytest.raises(capi.PhyhipError, match="Too many iterations in edge length optimization routine"):
            t.Br_Len_Opt(e, l=l0 * 20.0)
        t.s_opt.brent_it_max = capi.BRENT_IT_MAX
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(False)
        _restore(t, e, l0)
        # a NaN start: the floating-point error, nothing launched
        t.inst.profile(1)
        for bad in ((float("nan"), lkb), (l0, float("nan"))):
            with pytest.raises(capi.PhyhipError) as ei:
                t.inst.optimise_edge_length(bad[0], bad[1])
            assert ei.value.code == capi.ERROR_FLOATING_POINT
        for kw in (dict(iter_max=0), dict(iter_max=capi.BRENT_IT_MAX + 1), dict(tol=0.0)):
            with pytest.raises(capi.PhyhipError) as ei:
                t.inst.optimise_edge_length(l0, lkb, **kw)
            assert ei.value.code == capi.ERROR_OUT_OF_RANGE
        assert t.inst.profile_read_edge_length()[1:] == (0, 0)
        t.inst.profile(0)
    finally:
        t.close()


# ---- isolation -----------------------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing_but_the_warning():
    d = _golden("nucleic_gtr_g4")
    t, ot = device_tree_from_golden(d)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        ot.lk(None, both_sides=True)
        e = 7
        l0 = float(d["edge_len"][e])
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        lkb = t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        dot = t.inst.get_dot_prod()
        chain_before = [t.dLk(x, e) + (t.c_dlnL,) for x in (l0, l0 / 2, l0 * 3)]
        t.inst.profile(1)
        got = t.inst.optimise_edge_length(l0 * 20.0, lkb)
        ms, calls, evals = t.inst.profile_read_edge_length()
        t.inst.profile(0)
        assert calls == 1 and evals == got[3] and ms > 0.0
        assert t.inst.numerical_warning() == 0
        assert np.array_equal(t.inst.get_dot_prod(), dot)
        chain_after = [t.dLk(x, e) + (t.c_dlnL,) for x in (l0, l0 / 2, l0 * 3)]
        assert chain_before == chain_after           # the dLk chains on both sides of the call: the same bits
        t.Set_Use_Eigen_Lr(False)
        assert t.Lk(e) == lkb
        assert_device_state_is_the_oracles(t, ot, what="around phyhip_optimise_edge_length")
    finally:
        t.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_fall_back_to_the_chain():
    # a two-shard group, P one above the limit, a generic-loop instance: PHYHIP_ERROR_NO_IMPLEMENTATION; the host layer drives the chain
    for kw, p in ((dict(devices=[0, 0]), 300), (dict(), capi.BRLEN_MAX_PATTERNS + 1), (dict(use_m4mod=True), 300)):
        t, ot, tree, st = synthetic_pair(6, p, 4, 4, seed=5, **kw)
        try:
            t.Set_Both_Sides(True)
            t.Lk(None)
            e, l0 = 2, float(tree.edge_len[2])
            t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
            lkb = t.Lk(e)
            t.Set_Update_Eigen_Lr(False)
            with pytest.raises(capi.PhyhipError) as ei:
                t.inst.optimise_edge_length(l0, lkb)
            assert ei.value.code == capi.ERROR_NO_IMPLEMENTATION
            a = t.Br_Len_Opt(e, l=l0 * 5.0, force_device=True)
            assert not t.on_device
            _restore(t, e, l0)
            b = t.Br_Len_Opt(e, l=l0 * 5.0, force_host_chain=True)
            assert a == b and a[4] in (0, 1, 2) and a[3] >= 2
        finally:
            t.close()
    # a class-axis instance (the host layer's Lk / dLk do not serve one: mixture trees go through the class-mixture entry points)
    inst = capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True)
    try:
        with pytest.raises(capi.PhyhipError) as ei:
            inst.optimise_edge_length(0.1, -100.0)
        assert ei.value.code == capi.ERROR_NO_IMPLEMENTATION
    finally:
        inst.close()
