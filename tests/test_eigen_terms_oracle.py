"""The oracle side of tests/test_gpu_eigen_terms.py, without a GPU: what that file compares the device with is itself pinned here.

* orc.dlk_terms / orc.lk_eigen_terms (orc_dlk / orc_lk_eigen on one-pattern slices) added in site order ARE the whole-alignment
  sums, bit for bit -- on the golden fixtures' eigen edges and on every synthetic shape of the GPU file.
* Every class of the synthetic edge (eigen_terms.CLASSES) is there and takes its branch in the oracle: the floor's value and the
  warning, the exponent reset to 0 on an overflowing +I pattern, subnormal products with lk under the floor and dlk not 0.
* The oracle's per-pattern terms stay within the bounds of the exact reference (eigen_terms.Reference) -- the bounds the device is
  held to: derivative term gamma * (A_d / |lk| + |dlk| * A_l / lk^2), gamma = (S / 2 + C + 6) * 2^-53; lnL term gamma * A_l / lk
  carried through the log plus 3 spacings of max(|log lk|, LOG2 * fact)."""
import numpy as np
import pytest

import eigen_terms as et
import orc
from conftest import FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_slice_sums_are_the_whole_sums_on_the_fixtures(name, golden):
    d = golden(name)
    t = orc.tree_from_golden(d)
    t.lk(None, both_sides=True)
    for e in d["eigen_edges"]:
        e = int(e)
        t.lk(e); t.update_eigen_lr(e)
        for l in (float(t.len[e]), 0.003, 99.0):
            lc, lnl, dlnl = t.dlk(l)
            lc2, a, b = t.dlk_terms(l)
            assert lc2 == lc and orc.ordered_sum(a) == lnl and orc.ordered_sum(b) == dlnl, (name, e, l)
            assert orc.ordered_sum(t.lk_eigen_terms(l)) == t.lk_eigen(l), (name, e, l)
            assert not np.any(a[t.wght <= 0]) and not np.any(b[t.wght <= 0])


_cache = {}


def _edge(S, Cc, P, scaling=1):
    key = (S, Cc, P, scaling)
    if key not in _cache:
        E = et.make_edge(S, Cc, P, seed=1000 * S + 10 * Cc + P % 7, apply_scaling=scaling)
        _cache[key] = (E, et.oracle_edge(E), et.oracle_dot_prod(E))
    return _cache[key]


@pytest.mark.parametrize("S,Cc,P", et.SHAPES)
def test_slice_sums_are_the_whole_sums_on_the_synthetic_shapes(S, Cc, P):
    E, ev, dot = _edge(S, Cc, P)
    for l in (et.LENGTHS(et.L0) if P <= 300 else (et.L0, 99.0)):
        lc, lnl, dlnl, lnl_e = et.oracle_sums(E, l, E.wght, dot, ev["fact_sum_scale"])
        lc2, a, b, c = et.oracle_terms(E, l, E.wght, dot, ev["fact_sum_scale"], None)
        assert lc2 == lc == min(max(l, E.m.l_min), E.m.l_max)
        assert orc.ordered_sum(a) == lnl and orc.ordered_sum(b) == dlnl and orc.ordered_sum(c) == lnl_e, (l, lnl, dlnl)
        assert np.isfinite(lnl) and np.isfinite(dlnl)   # (the NaN partials sit in a pattern without weight)


@pytest.mark.parametrize("scaling", [1, 0])
@pytest.mark.parametrize("S", [4, 20])
def test_every_class_is_there_and_takes_its_branch(S, scaling):
    E, ev, dot = _edge(S, 4, 70, scaling)
    w = E.wght > 0
    n = {c: int((w & (E.cls == k)).sum()) for k, c in enumerate(et.CLASSES)}
    assert all(v >= 3 for c, v in n.items() if c != "nan_no_weight") and (E.cls == et.NAN_NO_WEIGHT).sum() >= 3, n
    assert set(np.unique(E.wght)) == {0.0, 1.0, 2.0}
    assert np.isnan(E.left[E.cls == et.NAN_NO_WEIGHT]).any() and np.isfinite(ev["lnL"])
    fact, site = ev["fact_sum_scale"], ev["c_lnL_sorted"]
    log_small = float(np.log(et.SMALL))
    # the floor, with its warning
    assert ev["warning"] == 1
    for k in (et.FLOOR, et.SUBNORMAL):
        assert np.all(site[w & (E.cls == k)] == log_small), et.CLASSES[k]
    assert np.all(site[w & (E.cls == et.ORDINARY)] > -50.0)
    # the exponents: reset to 0 where pi * 2^1280 overflows, kept elsewhere; all 0 with scaling off
    if scaling:
        assert np.all(fact[E.cls == et.INV_OVERFLOW] == 0) and np.all((E.sl + E.sr)[E.cls == et.INV_OVERFLOW] == 1280)
        assert np.all(fact[w & (E.cls == et.INV_SCALED)] == 256) and np.all(fact[w & (E.cls == et.SCALED)] == 256)
        m = E.cls == et.INV_OVERFLOW   # site_lk = pi * pinvar, no exponent left
        assert np.array_equal(site[m], np.log(E.m.pi[E.invar[m]] * E.m.pinvar))
    else:
        assert not np.any(fact)
    assert np.all(E.invar[np.isin(E.cls, (et.ORDINARY, et.FLOOR, et.SUBNORMAL, et.SCALED))] == -1) and E.m.invar_model == 1
    # subnormal products: entries of dot_prod under DBL_MIN but not 0, lk floored, a derivative that is not 0
    m = w & (E.cls == et.SUBNORMAL)
    assert np.all(np.abs(dot[m]) < et.SMALL) and np.all((dot[m] != 0.0).sum(axis=1) >= dot.shape[1] // 2)
    assert not np.any(dot[w & (E.cls == et.FLOOR)])
    _, a, b, c = et.oracle_terms(E, et.L0, E.wght, dot, fact, None)
    assert np.all(b[m] != 0.0) and np.all(a[m] == E.wght[m] * log_small) and not np.any(b[w & (E.cls == et.FLOOR)])
    # +I patterns: lk is at least pi * pinvar (times 2^fact where the exponent was kept)
    for k in (et.INV_SCALED, et.INV_UNSCALED, et.INV_OVERFLOW):
        m = w & (E.cls == k)
        assert np.all(c[m] / E.wght[m] + et.LOG2 * fact[m] >= np.log(E.m.pi[E.invar[m]] * E.m.pinvar) - 1e-9), et.CLASSES[k]


@pytest.mark.parametrize("S,Cc,P", et.SHAPES)
def test_the_oracle_stays_within_the_exact_references_bounds(S, Cc, P):
    E, ev, dot = _edge(S, Cc, P)
    fact = ev["fact_sum_scale"]
    probes = et.probe_list(E, et.tile_of(S, Cc))
    if P > 300:
        probes = probes[::7]   # (the oracle has no tiles: a seventh of the GPU file's probes)
    worst = [0.0, 0.0, 0.0]
    for l in et.LENGTHS(et.L0):
        ref = et.Reference(E, l)
        lc, a, b, c = et.oracle_terms(E, l, E.wght, dot, fact, probes)
        assert lc == ref.l
        for p in probes:
            wt = float(E.wght[p])
            t_l, t_d, b_d, b_l, _ = ref.dlk(dot[p], fact[p], int(E.invar[p]), wt)
            t_e, b_e, _ = ref.lk_eigen(dot[p], fact[p], int(E.invar[p]), wt)
            assert abs(b[p] - t_d) <= b_d, (p, l, et.CLASSES[E.cls[p]], b[p], t_d, b_d)
            assert abs(a[p] - t_l) <= b_l, (p, l, et.CLASSES[E.cls[p]], a[p], t_l, b_l)
            assert abs(c[p] - t_e) <= b_e, (p, l, et.CLASSES[E.cls[p]], c[p], t_e, b_e)
            for i, (x, y) in enumerate(((abs(b[p] - t_d), b_d), (abs(a[p] - t_l), b_l), (abs(c[p] - t_e), b_e))):
                if y > 0:
                    worst[i] = max(worst[i], x / y)
    print("largest error / bound (dlnL term, lnL term, eigen-basis lnL term):", worst)
    assert max(worst) > 0.0   # (the reference is not the oracle restated)


@pytest.mark.parametrize("S", [4, 20])
def test_the_restated_mixture_combinations_stay_within_the_exact_references_bounds(S):
    """phyml_amd.replay.mixture_combine / mixture_dlk (pinned to the reference's dumps by tests/test_mixture_oracle.py) pattern by
    pattern against eigen_terms.MixReference on the three-class input of the GPU file; every class of pattern is there, and an
    exponent sum of 1024 drops its class (pow(2, 1024) = inf) while 1025 is capped to 1023."""
    from phyml_amd import replay
    M = et.make_mix(S)
    w = M.wght > 0
    assert all(int((w & (M.cls == k)).sum()) >= 3 for k in range(len(et.MIX_CLASSES)) if k != et.M_NAN) and (M.cls == et.M_NAN).sum() >= 3
    un, fa, dots = [], [], []
    for k in range(M.K):
        E = et.mix_class_edge(M, k)
        ev = et.oracle_edge(E)
        un.append(ev["unscaled_site_lk_cat"][:, 0]); fa.append(ev["fact_sum_scale"]); dots.append(et.oracle_dot_prod(E))
    assert set(np.unique(fa[0][w])) == {0, 300, 1024, 1025}
    factors = list(zip(M.proba, M.r_w, M.e_w))
    models = [dict(l_min=[m.l_min], l_max=[m.l_max], br_len_mult=[m.br_len_mult], gamma_rr=m.gamma_rr, e_val=m.e_val) for m in M.models]
    for l in (et.L0, 99.0):
        ref = et.MixReference(M, l, 0)
        for p in np.nonzero(w)[0]:
            with np.errstate(over="ignore"):
                _, logs = replay.mixture_combine([u[p:p + 1] for u in un], [f[p:p + 1] for f in fa], factors, M.r_sum, M.e_sum, M.sum_probas, np.ones(1))
                a, d = replay.mixture_dlk([x[p:p + 1] for x in dots], [f[p:p + 1] for f in fa], models, factors, M.r_sum, M.e_sum, M.sum_probas, np.ones(1), l)
            t, b = ref.combine([u[p] for u in un], [f[p] for f in fa], -1, 1.0)
            tl, td, bl, bd = ref.dlk([x[p] for x in dots], [f[p] for f in fa], -1, 1.0)
            assert abs(logs[0] - t) <= b and abs(a - tl) <= bl and abs(d - td) <= bd, (p, et.MIX_CLASSES[M.cls[p]], l)
            if M.cls[p] == et.M_1024:   # class 0 (2^1000 before the scaling) is gone: the other two classes alone
                t2, _ = ref.combine([0.0] + [u[p] for u in un[1:]], [0] + [f[p] for f in fa[1:]], -1, 1.0)
                assert t2 == t
