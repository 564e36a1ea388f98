"""Per-pattern parity of the eigen-basis evaluations (phyhip_calculate_eigen_lnl_dlnl / phyhip_calculate_eigen_lnl: PhyML's dLk and the
eigen-basis Lk) and the rare branches of Lk_Core's tail on the routes a search runs.

A per-pattern term is seen through the public surface: the edge is evaluated and phyhip_update_eigen_lr run under the real
weights, then the weight vector is ONE-HOT (phyhip_set_pattern_weights) -- every other pattern adds 0.0, so the two returned sums
ARE pattern p's terms, whatever the order of summation.  Most probes use weight 1.0, every fifth 3.0.

What is held, per probe and per length (eigen_terms.LENGTHS: -1 -> l_min, 1e-9, l0 / 3, l0, 3 l0, 99 (len * rate beyond l_max for
some categories), 1e3 -> l_max):
  * the returned length is the oracle's;
  * the derivative term is np.array_equal to the oracle's (orc_dlk on the one-pattern slice of the device's own read-back
    dot_prod and the exponents the edge evaluation left): the same fused chain, the same table, the category sum in order, IEEE
    division;
  * the lnL term (of dLk and of the eigen-basis Lk) is within wt * 3 * spacing(max(|log lk|, LOG2 * fact)) of the oracle's: one ulp
    for each of the two log() and one for the subtraction.  (1 ulp for the device library's log is the figure the bound was
    specified with; no accuracy table of the device libraries ships with the toolchain to quote another.);
  * both terms are within the bounds of the exact reference (eigen_terms.Reference; tests/test_eigen_terms_oracle.py holds the
    oracle to the same): |d(dlk / lk)| <= gamma * (A_d / |lk| + |dlk| * A_l / lk^2), gamma = (S / 2 + C + 6) * 2^-53,
    A_l = sum_c w_c sum_s |dp * ex|, A_d = sum_c w_c sum_s |dp * ex * ev * rr|; the lnL term: gamma * A_l / lk carried through the
    log plus the three spacings.  (Subnormal results round absolutely, 2^-1075 each: Reference adds that share.)  The floor is
    applied in the reference too;
  * every form that serves the shape returns the same pair of doubles: launched against resident, one-shot against per-tile.

Which form ran is asserted from the resident evaluators' counters around the calls of every probe (commands answered by resident
workgroups: all of them, or none with PHYHIP_RESIDENT=0).  WHICH kernel a launched evaluation is follows from the shape alone (eigen_eval,
phyhip_eigen.hip) and is restated in launched_form(): the library keeps no counter per launched kernel.

The mixture kernels (mixture_combine_kernel, mixture_dlk_kernel) are held the same way by test_mixture_terms, in both layouts.

dlk_lane's own overflow branch (`issue`: lk = inf * pinvar, dlk = 0) is NOT reachable through the call sequences of the
reference: the edge evaluation that leaves the exponents resets an overflowing +I pattern's exponent to 0 first (asserted
below), so the dLk that follows sees 0.  (Switching the invariant model on between the two calls would reach it; no caller does.)

Probe counts: up to 300 patterns every pattern that carries weight; beyond, first and last pattern of every tile, the last
pattern, every special pattern and 128 random ones (4 x 4 x 1500: 237, 2100 patterns: 292, 4200: 343, 8161: 778), each at 7 lengths
on every form.  Wall time of the file on an MI355X: 29 s for its 42 cases; the slowest are the first sharded case (7.4 s, of which
5.5 s are the process's first RCCL communicator -- whichever file creates the first sharded instance pays it) and the one-shot
case (2.8 s, three forms x 778 probes); every other case takes 1.5 s or less."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import eigen_terms as et
import orc
from phyml_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = et.LENGTHS(et.L0)
# The one-shot large-grid launch needs dgrid > big_device_sum (200 tiles) and the group sum, i.e. as many workgroups as the
# device has CUs up to kBigGroupWgs = 256 (phyhip_host.hpp: big_sum_by_group; big_wgs = min(CUs, tiles)): 256 tiles of 32
# patterns (two lanes per pattern) -- the smallest P whose padded length is 8192
ONE_SHOT_P = 8161


def device_edge(E, devices=None, lib=None):
    """The edge on the device: buffers 2 / 3 with their exponents, matrix 0, the model block.  lib: another build of the library."""
    if lib is not None:
        L = C.CDLL(lib); L.phyhip_get_last_error.restype = C.c_char_p
        keep, capi._lib = capi._lib, L
    try:
        inst = capi.Instance(2, 4, E.S, E.P, 1, E.C, devices=devices)
    finally:
        if lib is not None:
            capi._lib = keep
    m = E.m
    inst.set_phyml_options(m.l_min, m.l_max, m.br_len_mult, E.apply_scaling)
    inst.set_pattern_weights(E.wght); inst.set_category_rates(m.gamma_rr); inst.set_category_weights(m.gamma_r_proba)
    inst.set_state_frequencies(m.pi); inst.set_eigen_decomposition(m.r_e_vect, m.l_e_vect, m.e_val)
    inst.set_invariant_sites(m.invar_model, m.pinvar, E.invar)
    inst.set_transition_matrix(0, E.pm)
    inst.set_partials(2, E.left); inst.set_partials(3, E.rght)
    for b, s in ((2, E.sl), (3, E.sr)):
        capi._chk(inst.L.phyhip_set_scale_factors(inst.id, b, capi._ptr(s)))
    return inst


def _chk(inst, rc):
    if rc < 0:
        raise capi.PhyhipError(f"phyhip error {rc}: {inst.L.phyhip_get_last_error().decode()}")


def answered(inst, which):
    """commands the resident workgroups answered: which = 0 the dLk evaluator, 1 the short-evaluation one, 2 the large-grid one"""
    if which == 2:
        o = (C.c_longlong * 4)(); _chk(inst, inst.L.phyhip_get_big_resident_stats(inst.id, o))
        return int(o[0] - o[2])
    o = (C.c_longlong * 8)(); _chk(inst, inst.L.phyhip_get_resident_stats(inst.id, o))
    return int(o[4 * which] - o[4 * which + 2])


def big_shape(S, Cc, P):
    """phyhip_host.hpp: big_shape -- more than 64 tiles of the lane-per-pattern kernel"""
    return S == 4 and Cc <= 4 and ((P + 63) // 64 * 64) // et.tile_of(S, Cc) > 64


def launched_form(S, Cc, P):
    if big_shape(S, Cc, P):
        return "one-shot large-grid launch" if P >= ONE_SHOT_P and Cc % 2 == 0 else "dlk64_kernel"
    return "dlk_kernel"


def resident_serves(S, Cc, P):
    """eigen_eval: the resident dLk evaluator takes 4 states (20: the table from the edge length, up to 8 categories) with the table
    in the kernel arguments and at most 64 workgroups; big shapes go to the large-grid evaluator"""
    if big_shape(S, Cc, P):
        return True
    cp = 1 << (Cc - 1).bit_length()
    return (S == 4 or Cc <= 8) and Cc * 2 * S <= 320 and (P * cp + 255) // 256 <= 64


def evaluate_edge(inst, E, repeat=1):
    """The edge evaluation of the hot path and what it left; then Update_Eigen_Lr and its products.  repeat: evaluations in a row
    (the resident evaluators take over a call sequence, not its first call)."""
    out = {}
    for _ in range(repeat):
        before = answered(inst, 1) + answered(inst, 2)
        out["lnL"] = inst.edge_lnl(2, 3, 0)
        out["resident"] = answered(inst, 1) + answered(inst, 2) - before
    out["warning"] = inst.numerical_warning()
    out["c_lnL_sorted"], out["cur_site_lk"], out["unscaled_site_lk_cat"], out["fact_sum_scale"] = inst.site_outputs()
    inst.update_eigen_lr(2, 3)
    out["dot_prod"] = inst.get_dot_prod()
    return out


def probe(inst, E, probes, warm=0):
    """One-hot weights pattern by pattern, every length: arrays [probe][length] of the returned length, the two sums of dLk and the
    eigen-basis lnL, and per probe how many commands resident workgroups answered (one per call and shard).  warm: evaluations thrown away after each weight change (the
    large-grid evaluator is launched at the second call of a sequence)."""
    n = (len(probes), len(LENGTHS))
    r = dict(l=np.zeros(n), lnl=np.zeros(n), dlnl=np.zeros(n), lnl_e=np.zeros(n), answered=np.zeros(len(probes), int))
    w = np.zeros(E.P)
    count = lambda: answered(inst, 0) + answered(inst, 2)  # noqa: E731
    for i, p in enumerate(probes):
        w[:] = 0.0; w[p] = et.probe_weight(p)
        inst.set_pattern_weights(w)
        inst.synchronize()   # (the upload has arrived: the stream is idle, resident workgroups may take the next call)
        for _ in range(warm):
            inst.eigen_lnl_dlnl(et.L0)
        c0 = count()
        for j, l in enumerate(LENGTHS):
            r["l"][i, j], r["lnl"][i, j], r["dlnl"][i, j] = inst.eigen_lnl_dlnl(l)
            r["lnl_e"][i, j] = inst.eigen_lnl(l)
        r["answered"][i] = count() - c0
    inst.set_pattern_weights(E.wght)
    return r


def by_class(E, probes, bad):
    """which probes failed, for the assertion message: {class: count}, the first (pattern, length)"""
    i, j = np.nonzero(bad)
    if len(i) == 0:
        return None
    n = {}
    for k in i:
        c = et.CLASSES[E.cls[probes[k]]]; n[c] = n.get(c, 0) + 1
    return n, ("pattern", int(probes[i[0]]), "length", LENGTHS[j[0]])


def check_edge_outputs(E, ev, oracle, exact=None, what=None):
    """What the hot-path edge evaluation left against the oracle (and the exact route on the same instance)."""
    w = E.wght > 0
    refs = [("oracle", oracle["c_lnL_sorted"], oracle["unscaled_site_lk_cat"], oracle["fact_sum_scale"], oracle["warning"])]
    if exact is not None:
        refs.append(("exact route", exact[0], exact[2], exact[3], exact[5]))
    for name, site, cat, fact, warn in refs:
        # the exponents, the reset to 0 on an overflowing +I pattern included, and the warning
        assert np.array_equal(ev["fact_sum_scale"][w], fact[w]), (what, name)
        assert ev["warning"] == warn, (what, name)
        # the category likelihoods: the fixtures' rtol (not array_equal: the hot path takes the general product where the
        # reference takes the tip branch, and its own operation order in the 20-state kernel)
        assert np.allclose(ev["unscaled_site_lk_cat"][w], cat[w], rtol=1e-12, atol=0), (what, name)
        f = fact[w].astype(np.float64)
        log_lk = site[w] + et.LOG2 * f
        tol = 1e-12 + 3 * np.spacing(np.maximum(np.abs(log_lk), et.LOG2 * f))
        err = np.abs(ev["c_lnL_sorted"][w] - site[w])
        assert np.all(err <= tol), (what, name, float(np.max(err / tol)))
    assert np.all(ev["fact_sum_scale"][E.cls == et.INV_OVERFLOW][w[E.cls == et.INV_OVERFLOW]] == 0) or not E.apply_scaling
    # the scalar: the ordered sum of the weighted terms, to P spacings (block sums add in another order)
    s = orc.ordered_sum(E.wght[w] * ev["c_lnL_sorted"][w])
    assert np.isfinite(ev["lnL"]) and abs(ev["lnL"] - s) <= E.P * np.spacing(abs(s)), (what, ev["lnL"], s)


_refs = {}


def references(E, key, dot, fact, probes):
    """Oracle and exact-reference terms of the probes under their one-hot weights, once per case: arrays [probe][length]"""
    if key in _refs:
        return _refs[key]
    n = (len(probes), len(LENGTHS))
    o = dict(l=np.zeros(n), lnl=np.zeros(n), dlnl=np.zeros(n), lnl_e=np.zeros(n))
    x = dict(lnl=np.zeros(n), dlnl=np.zeros(n), lnl_e=np.zeros(n), b_lnl=np.zeros(n), b_dlnl=np.zeros(n), b_lnl_e=np.zeros(n), sp=np.zeros(n))
    w = np.zeros(E.P)
    for p in probes:
        w[p] = et.probe_weight(p)
    for j, l in enumerate(LENGTHS):
        lc, a, b, c = et.oracle_terms(E, l, w, dot, fact, probes)
        o["l"][:, j], o["lnl"][:, j], o["dlnl"][:, j], o["lnl_e"][:, j] = lc, a[probes], b[probes], c[probes]
        ref = et.Reference(E, l)
        for i, p in enumerate(probes):
            wt, f, iv = float(w[p]), int(fact[p]), int(E.invar[p])
            x["lnl"][i, j], x["dlnl"][i, j], x["b_dlnl"][i, j], x["b_lnl"][i, j], loglk = ref.dlk(dot[p], f, iv, wt)
            x["lnl_e"][i, j], x["b_lnl_e"][i, j], loglk_e = ref.lk_eigen(dot[p], f, iv, wt)
            x["sp"][i, j] = wt * 3 * np.spacing(max(abs(loglk), abs(loglk_e), et.LOG2 * f))
    _refs.clear()   # (one case at a time)
    _refs[key] = (o, x)
    return o, x


def check_terms(E, probes, r, o, x, what):
    """One form's probes against the oracle and the exact reference."""
    assert np.array_equal(r["l"], o["l"]), (what, "returned length")
    bad = ~((r["dlnl"] == o["dlnl"]) | (np.isnan(r["dlnl"]) & np.isnan(o["dlnl"])))
    assert not bad.any(), (what, "derivative term differs from the oracle's", by_class(E, probes, bad),
                           float(np.nanmax(np.abs(r["dlnl"] - o["dlnl"]) / np.maximum(np.abs(o["dlnl"]), 1e-300))))
    for k in ("lnl", "lnl_e"):
        bad = ~(np.abs(r[k] - o[k]) <= x["sp"])
        assert not bad.any(), (what, k + " term against the oracle", by_class(E, probes, bad))
    for k in ("dlnl", "lnl", "lnl_e"):
        bad = ~(np.abs(r[k] - x[k]) <= x["b_" + k])
        assert not bad.any(), (what, k + " term against the exact reference", by_class(E, probes, bad))


def run_forms(E, key, forms, monkeypatch, oracle=None, with_exact=False):
    """forms: [(name, environment, keyword arguments of device_edge, commands resident workgroups answer per call)].  Every form is evaluated, probed and
    checked; all forms must return the same doubles."""
    probes = et.probe_list(E, et.tile_of(E.S, E.C))
    oracle = oracle or et.oracle_edge(E)
    first = None
    for name, env, kw, resident in forms:
        t0 = time.perf_counter()
        for k in ("PHYHIP_RESIDENT", "PHYHIP_SHARD_HOST_COMBINE", "PHYHIP_BIG_ONE_SHOT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        inst = device_edge(E, **kw)
        try:
            ev = evaluate_edge(inst, E)
            exact = inst.exact_site_outputs(2, 3, 0) if with_exact else None
            check_edge_outputs(E, ev, oracle, exact, (key, name))
            r = probe(inst, E, probes, warm=1 if (resident and big_shape(E.S, E.C, E.P)) else 0)
        finally:
            inst.close()
        # the form that ran: every call answered by resident workgroups (on every shard), or none
        n_res = int(resident) * 2 * len(LENGTHS)
        assert np.all(r["answered"] == n_res), (key, name, "commands answered per probe, expected", n_res, np.unique(r["answered"]))
        o, x = references(E, key, ev["dot_prod"], ev["fact_sum_scale"], probes)
        check_terms(E, probes, r, o, x, (key, name))
        print(f"{key} {name}: {len(probes)} probes, {time.perf_counter() - t0:.2f} s")
        if first is None:
            first = (name, ev, r)
        else:
            assert np.array_equal(ev["dot_prod"], first[1]["dot_prod"], equal_nan=True) and np.array_equal(ev["fact_sum_scale"], first[1]["fact_sum_scale"])
            for k in ("l", "lnl", "dlnl", "lnl_e"):
                assert np.array_equal(r[k], first[2][k], equal_nan=True), (key, name, "against", first[0], k)
    return len(probes)


def _edge(S, Cc, P, scaling=1):
    return et.make_edge(S, Cc, P, seed=1000 * S + 10 * Cc + P % 7, apply_scaling=scaling)


def plain_forms(S, Cc, P):
    forms = [(launched_form(S, Cc, P), {"PHYHIP_RESIDENT": "0"}, {}, False)]
    if resident_serves(S, Cc, P):
        forms.append(("resident", {"PHYHIP_RESIDENT": "1"}, {}, True))
    return forms


# ---- 1: the forms of the evaluation, at the smallest shapes that select them -----------------------------------------------------
PLAIN = [(4, 4, 1), (4, 4, 70), (4, 3, 65), (4, 1, 130), (4, 2, 257), (4, 5, 70), (4, 8, 70), (4, 40, 70),   # dlk_kernel, resident_dlk_kernel
         (4, 4, 1500),                                      # resident_dlk_kernel relaying the command through device memory
         (4, 64, 70), (20, 12, 40),                         # the table through device memory (launched only)
         (4, 4, 2100), (4, 2, 2100),                        # dlk64_kernel / large-grid resident workgroups, two lanes per pattern
         (4, 3, 4200), (4, 1, 4200),                        # ... one lane per pattern
         (20, 4, 70), (20, 1, 33), (20, 3, 17), (20, 8, 40)]  # 20 states, the table from the edge length, launched and resident


@pytest.mark.parametrize("S,Cc,P", PLAIN)
def test_per_pattern_terms(S, Cc, P, monkeypatch):
    forms = plain_forms(S, Cc, P)
    assert (len(forms) == 2) == ((S, Cc, P) not in ((4, 64, 70), (20, 12, 40)))
    n = run_forms(_edge(S, Cc, P), (S, Cc, P), forms, monkeypatch)
    print(f"{S} x {Cc} x {P}: {n} probes x {len(LENGTHS)} lengths x {len(forms)} forms")


def test_per_pattern_terms_one_shot_launch(monkeypatch):
    """ONE_SHOT_P patterns: the launched evaluation is the one-shot large-grid launch (256 workgroups add per workgroup and post
    one record per sum), the resident one the same workgroups staying; the diag build with PHYHIP_BIG_ONE_SHOT=0 launches the
    per-tile form (dlk64_kernel) on the same shape."""
    S, Cc, P = 4, 4, ONE_SHOT_P
    assert launched_form(S, Cc, P) == "one-shot large-grid launch" and launched_form(S, Cc, P - 1) == "dlk64_kernel"
    diag = os.path.join(ROOT, "phyml_amd", "lib_diag", "libphyhip.so")
    assert os.path.exists(diag), "the diag build rides along with the product (__graft_entry__.build())"
    forms = plain_forms(S, Cc, P) + [("per-tile (diag build)", {"PHYHIP_RESIDENT": "0", "PHYHIP_BIG_ONE_SHOT": "0"}, {"lib": diag}, False)]
    n = run_forms(_edge(S, Cc, P), (S, Cc, P), forms, monkeypatch)
    print(f"{S} x {Cc} x {P}: {n} probes x {len(LENGTHS)} lengths x {len(forms)} forms")


@pytest.mark.parametrize("S,Cc,P,shards", [(4, 4, 300, 3), (20, 4, 90, 2)])
def test_per_pattern_terms_sharded(S, Cc, P, shards, monkeypatch):
    """Shards on device 0: the shards' own evaluations added on the host in shard order (their resident evaluators serve them), and
    the fused device sum + all-reduce (nothing resident)."""
    devs = {"devices": [0] * shards}
    forms = [("unsharded", {"PHYHIP_RESIDENT": "0"}, {}, False),
             ("host sum", {"PHYHIP_RESIDENT": "1", "PHYHIP_SHARD_HOST_COMBINE": "1"}, devs, shards),
             ("device sum + all-reduce", {"PHYHIP_RESIDENT": "1", "PHYHIP_SHARD_HOST_COMBINE": "0"}, devs, False)]
    run_forms(_edge(S, Cc, P), (S, Cc, P, "sharded"), forms, monkeypatch)


# ---- 2: the tail's branches on the routes a search uses ----------------------------------------------------------------------------
TAILS = [(4, 4, "traverse_nt2_kernel"), (4, 3, "traverse_nt2_kernel"), (20, 4, "20-state kernel"), (20, 1, "20-state kernel"),
         (4, 5, "generic kernel"), (4, 12, "generic kernel"), (20, 5, "generic kernel"), (20, 12, "generic kernel"),
         # (the tail is instantiated per category count)
         (4, 2, "traverse_nt2_kernel"), (4, 1, "traverse_nt2_kernel"), (20, 2, "20-state kernel"), (20, 3, "20-state kernel")]


@pytest.mark.parametrize("scaling", [1, 0])
@pytest.mark.parametrize("S,Cc,kernel", TAILS)
def test_tail_branches_on_the_hot_path(S, Cc, kernel, scaling, monkeypatch):
    """70 patterns of every class (eigen_terms.CLASSES; weights 0, 1, 2; a pattern without weight carries NaN) through
    phyhip_calculate_edge_log_likelihoods + phyhip_get_site_outputs, launched and -- where the shape has one -- by the resident
    short-evaluation workgroups; against phyhip_calculate_edge_site_outputs_exact on the same instance and against the oracle.
    fact_sum_scale (the reset to 0 on +I overflow included) and the warning are equal; unscaled_site_lk_cat agrees at
    rtol = 1e-12 (allclose, not array_equal: see check_edge_outputs); c_lnL_sorted within 1e-12 + 3 spacings; the scalar is the
    ordered sum of the terms within P spacings.  Then Update_Eigen_Lr and the one-hot probes of part 1 on the same buffers: the dLk
    after an overflow sees the reset exponent."""
    E = _edge(S, Cc, 70, scaling)
    oracle = et.oracle_edge(E)
    assert oracle["warning"] == 1
    w = E.wght > 0
    has_resident = kernel != "generic kernel"
    for res in (("0", "1") if has_resident else ("0",)):
        monkeypatch.setenv("PHYHIP_RESIDENT", res)
        inst = device_edge(E)
        try:
            ev = evaluate_edge(inst, E, repeat=3)
            assert (ev["resident"] > 0) == (res == "1"), (kernel, res, ev["resident"])
            check_edge_outputs(E, ev, oracle, inst.exact_site_outputs(2, 3, 0), (S, Cc, kernel, scaling, res))
            assert np.all(ev["c_lnL_sorted"][w & (E.cls == et.FLOOR)] < -708.0) and np.all(ev["c_lnL_sorted"][w & (E.cls == et.ORDINARY)] > -50.0)
        finally:
            inst.close()
    n = run_forms(E, (S, Cc, 70, scaling, "tail"), plain_forms(S, Cc, 70), monkeypatch, oracle=oracle, with_exact=True)
    assert n == int(w.sum())


# ---- 3: mixtures -------------------------------------------------------------------------------------------------------------------
def _da(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def _ia(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


class DeviceMixture:
    """The three classes of eigen_terms.make_mix as list entries of phyhip_calculate_mixture_*: one instance per class
    (layout "instances"), or classes on the category axis (layout "axis": 20 states all three on one instance, nucleotides two on a
    class-axis instance and the third as a plain one -- a class-axis nucleotide instance holds 1, 2 or 4 classes)."""

    def __init__(self, M, layout):
        self.M, S, P = M, M.S, M.P
        groups = [[0], [1], [2]] if layout == "instances" else ([[0, 1, 2]] if S == 20 else [[0, 1], [2]])
        self.groups, self.inst = groups, []
        for g in groups:
            axis = layout == "axis" and len(g) > 1
            inst = capi.Instance(2, 4, S, P, 1, len(g), class_axis=axis)
            self.inst.append(inst)
            m = M.models[g[0]]
            inst.set_phyml_options(m.l_min, m.l_max, m.br_len_mult, 1)
            inst.set_pattern_weights(M.wght); inst.set_category_rates([M.rates[k] for k in g]); inst.set_category_weights(np.full(len(g), 1.0 / len(g)))
            for j, k in enumerate(g):
                if j == 0 or axis:
                    inst.set_state_frequencies(M.models[k].pi, index=j)
                    inst.set_eigen_decomposition(M.models[k].r_e_vect, M.models[k].l_e_vect, M.models[k].e_val, index=j)
            inst.set_invariant_sites(0, 0.0, None)
            inst.set_transition_matrix(0, np.concatenate([M.pm[k] for k in g]))
            inst.set_partials(2, np.concatenate([M.left[k] for k in g], axis=1)); inst.set_partials(3, np.concatenate([M.rght[k] for k in g], axis=1))
            if g[0] == 0:   # (the exponents of class 0: the first class of the first entry)
                for b, s in ((2, M.sl), (3, M.sr)):
                    capi._chk(inst.L.phyhip_set_scale_factors(inst.id, b, capi._ptr(s)))
        self.ids = [i.id for i in self.inst]
        self.tab = (_da(M.proba), _da(M.r_w), _da(M.e_w), C.c_double(M.r_sum), C.c_double(M.e_sum), C.c_double(M.sum_probas))

    def close(self):
        for i in self.inst:
            i.close()

    def set_weights(self, w):
        for i in self.inst:
            i.set_pattern_weights(w)

    def set_invariant(self, on):
        M = self.M
        capi._chk(self.inst[0].L.phyhip_set_mixture_invariant_sites(self.ids[0], int(on), C.c_double(M.pinvar), capi._ptr(M.invar), capi._ptr(orc.f64(M.models[0].pi))))

    def lnl(self):
        n, out = len(self.ids), C.c_double(0.0)
        capi._chk(self.inst[0].L.phyhip_calculate_mixture_log_likelihood(_ia(self.ids), n, _ia([2] * n), _ia([3] * n), _ia([0] * n), *self.tab, C.byref(out)))
        return out.value, self.inst[0].numerical_warning()

    def dlk(self, l):
        n, lv, a, b = len(self.ids), C.c_double(l), C.c_double(0.0), C.c_double(0.0)
        capi._chk(self.inst[0].L.phyhip_calculate_mixture_eigen_lnl_dlnl(_ia(self.ids), n, _ia([2] * n), _ia([3] * n), C.byref(lv), *self.tab, C.byref(a), C.byref(b)))
        return lv.value, a.value, b.value, self.inst[0].numerical_warning()

    def class_outputs(self):
        """per class: unscaled likelihood [P], exponent [P] of the last edge evaluations, products [P][S] of Update_Eigen_Lr"""
        un, fa, dots = [], [], []
        for g, inst in zip(self.groups, self.inst):
            _, _, u, f = inst.site_outputs(n_fact=len(g))
            d = inst.get_dot_prod()
            for j in range(len(g)):
                un.append(u[:, j].copy()); fa.append(f.reshape(len(g), -1)[j].copy()); dots.append(d[:, j * self.M.S:(j + 1) * self.M.S].copy())
        return un, fa, dots


@pytest.mark.parametrize("layout", ["instances", "axis"])
@pytest.mark.parametrize("S", [4, 20])
def test_mixture_terms(S, layout):
    """mixture_combine_kernel (MIXT_Lk) and mixture_dlk_kernel (MIXT_dLk), three classes, 70 patterns, one-hot probes over every
    pattern with weight: against the exact reference (eigen_terms.MixReference) with +I, and without +I also against the restated
    combinations tests/test_gpu_mixture.py uses (phyml_amd.replay.mixture_combine / mixture_dlk on the pattern's slice; they and the
    device are both within the exact reference's bound, so within twice the bound of each other).  Exponent sums of 1024 pass
    through -- pow(2, 1024) is inf in the reference, the class drops out of the sum -- and 1025 is capped to 1023 with the warning
    (src/mixt.c:1040-1051, :3180-3197).  The warning: MIXT_Lk tests the exponent sums of every pattern, weight or not (:1029-1047 lie
    outside the weight test), so it is raised at every probe here; MIXT_dLk tests them inside the weight test (:3144-3198), so a probe
    raises it exactly when its own pattern is capped."""
    from phyml_amd import replay
    M = et.make_mix(S)
    factors = list(zip(M.proba, M.r_w, M.e_w))
    models = [dict(l_min=[m.l_min], l_max=[m.l_max], br_len_mult=[m.br_len_mult], gamma_rr=m.gamma_rr, e_val=m.e_val) for m in M.models]
    D = DeviceMixture(M, layout)
    try:
        D.set_invariant(1)
        lnl, warn = D.lnl()
        assert np.isfinite(lnl) and warn == 1            # (the NaN partials sit in a pattern without weight; sums of 1025 are there)
        for inst in D.inst:
            inst.update_eigen_lr(2, 3)
        un, fa, dots = D.class_outputs()
        w_all = M.wght > 0
        # the classes' own pieces are the oracle's: exponents equal, likelihoods at the fixtures' rtol
        for k in range(M.K):
            ev = et.oracle_edge(et.mix_class_edge(M, k))
            assert np.array_equal(fa[k][w_all], ev["fact_sum_scale"][w_all]) and np.allclose(un[k][w_all], ev["unscaled_site_lk_cat"][w_all, 0], rtol=1e-12, atol=0)
        assert set(np.unique(fa[0][w_all])) == {0, 300, 1024, 1025} and not np.any(fa[1]) and not np.any(fa[2])
        refs = {(l, inv): et.MixReference(M, l, inv) for l in LENGTHS for inv in (0, 1)}
        w = np.zeros(M.P)
        failed = []

        def hold(ok, *msg):
            if not ok:
                failed.append(msg)
        for p in np.nonzero(w_all)[0]:
            wt = et.probe_weight(p)
            w[:] = 0.0; w[p] = wt
            D.set_weights(w)
            capped = fa[0][p] > 1024
            for inv in (1, 0):
                D.set_invariant(inv)
                iv = int(M.invar[p]) if inv else -1
                what = (S, layout, int(p), et.MIX_CLASSES[M.cls[p]], "+I" if inv else "no +I")
                got, warn = D.lnl()
                t, b = refs[(et.L0, inv)].combine([u[p] for u in un], [f[p] for f in fa], iv, wt)
                hold(abs(got - t) <= b, what, "MIXT_Lk", got, t, b)
                hold(warn == 1, what, "MIXT_Lk warning", warn)   # (MIXT_Lk tests the sums of every pattern, weight or not: :1029-1047)
                if not inv:
                    with np.errstate(over="ignore"):
                        _, logs = replay.mixture_combine([u[p:p + 1] for u in un], [f[p:p + 1] for f in fa], factors, M.r_sum, M.e_sum, M.sum_probas, w[p:p + 1])
                    hold(abs(got - wt * logs[0]) <= 2 * b, what, "MIXT_Lk against the restated combination", got, wt * logs[0])
                for l in LENGTHS:
                    ref = refs[(l, inv)]
                    lc, a, d, warn = D.dlk(l)
                    tl, td, bl, bd = ref.dlk([x[p] for x in dots], [f[p] for f in fa], iv, wt)
                    hold(lc == ref.l, what, "returned length", l)
                    hold(abs(a - tl) <= bl and abs(d - td) <= bd, what, "MIXT_dLk", l, (a, tl, bl), (d, td, bd))
                    hold(warn == int(capped), what, "MIXT_dLk warning", warn)
                    if not inv:
                        with np.errstate(over="ignore"):
                            ra, rd = replay.mixture_dlk([x[p:p + 1] for x in dots], [f[p:p + 1] for f in fa], models, factors, M.r_sum, M.e_sum, M.sum_probas, w[p:p + 1], l)
                        hold(abs(a - ra) <= 2 * bl and abs(d - rd) <= 2 * bd, what, "MIXT_dLk against the restated combination", l, (a, ra), (d, rd))
        kinds = sorted({(m[0][3], m[0][4], m[1]) for m in failed})
        if failed:
            print("FAILED KINDS", kinds, [m for m in failed if m[1] != "MIXT_dLk warning"][:4])
        assert not failed, (len(failed), kinds[:16], failed[:2])
    finally:
        D.close()
