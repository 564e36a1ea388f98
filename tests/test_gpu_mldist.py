"""phyhip_calculate_pairwise_ml_distances (ML_Dist on the device) against the REAL reference's matrices (tests/golden/mldist_*.npz)
and against the restatement (tests/mldist_ref.py, itself held to the reference by tests/test_mldist_restatement.py).

Bounds: distances 1e-9 relative (the restatement's own distance from the reference binary is its compiler's contraction, 1e-10 at
worst; another branch of the optimiser lands orders of magnitude away); Lk_Dist at the answer 1e-10 relative (the project's
gate); iteration counts and, with integer weights, the counts: equal; starting values: the reference's bits on 4 states, 1e-14 on
20 states (contraction in 1 - c P)."""
import os

import numpy as np
import pytest

import mldist_ref as mr
import orc
from conftest import GOLDEN
from gpu_common import synthetic_pair
from phyml_amd import capi, workloads

pytestmark = pytest.mark.gpu

WANT = ("initial", "counts", "lnl", "iterations")
MDL = 1e-3


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(b), 1e-300)


def make_instance(chars, wght, mod, **kw):
    """A plain instance holding the tips, weights and model of an alignment (one rate category)"""
    chars = np.asarray(chars, dtype=np.uint8)
    n, P = chars.shape
    inst = capi.Instance(n, 2 * n, mod.ns, P, 2 * n, 1, **kw)
    inst.set_pattern_weights(wght)
    inst.set_category_rates([1.0]); inst.set_category_weights([1.0])
    inst.set_state_frequencies(mod.pi)
    inst.set_eigen_decomposition(mod.U, mod.V, mod.R)
    inst.set_phyml_options(mod.l_min, mod.l_max, 1.0, 1)
    for t in range(n):
        inst.set_tip_partials(t, orc.init_tip(0 if mod.ns == 4 else 1, chars[t])[0])
    return inst


def synth_model(ns):
    m = orc.Model(dict(workloads.model_block("model_gtr_g4" if ns == 4 else "model_lg_g4")))
    return mr.Model(m.pi, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max)


def synth_chars(n, P, ns, seed=5):
    """Related sequences from the integer hash, an ambiguous character every fifth cell (synthetic_pair's ambiguous_every)"""
    from phyml_amd import synth
    base = (synth.hash_u64(seed, 1, np.arange(P)) % np.uint64(ns)).astype(np.int64)
    chars = np.zeros((n, P), np.uint8)
    amb = np.frombuffer(b"N-RY?" if ns == 4 else b"X-?BZ", dtype=np.uint8)
    for t in range(n):
        hit = (synth.hash_u64(seed, 10 + t, np.arange(P)) % np.uint64(100)).astype(np.int64) < 10 + 5 * (t % 7)
        new = (synth.hash_u64(seed, 50 + t, np.arange(P)) % np.uint64(ns)).astype(np.int64)
        chars[t] = synth.states_to_chars(np.where(hit, new, base).astype(np.uint8), ns)
        idx = np.arange((t * 7) % 5, P, 5)
        chars[t, idx] = amb[(idx + t) % len(amb)]
    return chars


def check_against(got, extra, ref, counts_exact=True):
    """A device answer (distances, the optional arrays) against a restatement dict"""
    D = got
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    assert rel(D[iu], ref["dist"][iu]).max() < 1e-9, rel(D[iu], ref["dist"][iu]).max()
    assert np.array_equal(extra["iterations"], ref["iterations"])
    nz = ref["lnl"] != 0
    assert np.array_equal(extra["lnl"][~nz], ref["lnl"][~nz]) and (not nz.any() or rel(extra["lnl"][nz], ref["lnl"][nz]).max() < 1e-10)
    if counts_exact:
        assert np.array_equal(extra["counts"], ref["F"])


# the four fixtures ----------------------------------------------------------------------------------------------------------------
_fx = {}


def fixture_case(name):
    if name not in _fx:
        fx = dict(np.load(os.path.join(GOLDEN, "mldist_" + name + ".npz")))
        mod = mr.model_of(fx)
        ref = mr.ml_dist(fx["chars"], fx["wght"], mod, float(fx["min_diff_lk_local"][0]), start=fx["start"])
        _fx[name] = (fx, mod, ref)
    return _fx[name]


@pytest.mark.parametrize("name", ["nucleic", "proteic", "designed_nt", "designed_aa"])
def test_the_reference_matrices(name):
    fx, mod, ref = fixture_case(name)
    inst = make_instance(fx["chars"], fx["wght"], mod)
    try:
        D, extra = inst.pairwise_ml_distances(float(fx["min_diff_lk_local"][0]), want=WANT)
        n = D.shape[0]
        iu = np.triu_indices(n, 1)
        worst = rel(D[iu], fx["dist"][iu]).max()
        print(f"{name}: worst relative difference from the reference {worst:.3g}; from the restatement {rel(D[iu], ref['dist'][iu]).max():.3g}")
        assert worst < 1e-9
        check_against(D, extra, ref)
        S0 = extra["initial"]
        assert np.array_equal(S0, S0.T) and not S0.diagonal().any()
        if mod.ns == 4:
            assert np.array_equal(S0[iu], fx["start"][iu])
        else:
            assert rel(S0[iu], fx["start"][iu]).max() < 1e-14
        if name.startswith("designed"):
            at = lambda key: tuple(int(v) for v in fx["pair_" + key])
            assert D[at("identical")] == mod.l_min and D[at("disjoint")] == 0.1 and D[at("saturated")] == 2.0
            assert S0[at("disjoint")] == -1.0 and S0[at("saturated")] == -1.0 and S0[at("over")] == 2.0
        # the plain call returns the same matrix
        assert np.array_equal(inst.pairwise_ml_distances(float(fx["min_diff_lk_local"][0])), D)
    finally:
        inst.close()


# the smallest shapes at which the kernels can still go wrong -----------------------------------------------------------------------
SHAPES = [(4, n, P) for n in (2, 5, 13, 17) for P in (1, 3, 4, 5, 300)] + [(20, n, P) for n in (2, 7, 9) for P in (1, 3, 270)]


@pytest.mark.parametrize("ns,n,P", SHAPES)
def test_small_shapes(ns, n, P):
    mod = synth_model(ns)
    chars = synth_chars(n, P, ns)
    w = 1.0 + (np.arange(P) % 3)
    ref = mr.ml_dist(chars, w, mod, MDL)
    inst = make_instance(chars, w, mod)
    try:
        D, extra = inst.pairwise_ml_distances(MDL, want=WANT)
        check_against(D, extra, ref)
        if ns == 4:
            assert np.array_equal(extra["initial"], ref["start"])
        else:
            assert rel(extra["initial"], ref["start"]).max() < 1e-14
    finally:
        inst.close()


@pytest.mark.parametrize("ns,n,P", [(4, 17, 300), (20, 9, 270)])
def test_bands_of_taxa_change_nothing(ns, n, P):
    """A work space of one taxon's counts: every band holds one taxon, the counts are formed twice"""
    mod = synth_model(ns)
    chars = synth_chars(n, P, ns)
    w = 1.0 + (np.arange(P) % 3)
    inst = make_instance(chars, w, mod)
    try:
        D, extra = inst.pairwise_ml_distances(MDL, want=WANT)
        for nbytes in (1, 3 * ns * (n * ns + 64) * 8):
            inst.set_pairwise_work_space(nbytes)
            D2, e2 = inst.pairwise_ml_distances(MDL, want=WANT)
            assert np.array_equal(D, D2) and all(np.array_equal(extra[k], e2[k]) for k in WANT)
            D3 = inst.pairwise_ml_distances(MDL, initial=extra["initial"])
            assert np.array_equal(D, D3)
        inst.set_pairwise_work_space(0)
        assert np.array_equal(inst.pairwise_ml_distances(MDL), D)
    finally:
        inst.close()


# weights ---------------------------------------------------------------------------------------------------------------------------
def test_zero_weight_patterns(golden):
    d = golden("nucleic_zero_w")
    m = orc.Model(d)
    mod = mr.Model(m.pi, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max)
    assert np.any(d["wght"] == 0)
    ref = mr.ml_dist(d["tip_chars"], d["wght"], mod, MDL)
    inst = make_instance(d["tip_chars"], d["wght"], mod)
    try:
        D, extra = inst.pairwise_ml_distances(MDL, want=WANT)
        check_against(D, extra, ref)
        assert np.array_equal(extra["initial"], ref["start"])
    finally:
        inst.close()


@pytest.mark.parametrize("ns", [4, 20])
def test_reweighting_between_two_calls(ns):
    mod = synth_model(ns)
    n, P = (13, 300) if ns == 4 else (7, 270)
    chars = synth_chars(n, P, ns)
    w1 = 1.0 + (np.arange(P) % 3)
    w2 = np.where(np.arange(P) % 4 == 1, 0.0, 1.0 + (np.arange(P) % 5))   # (a bootstrap replicate: some patterns drop out)
    a, b = make_instance(chars, w1, mod), make_instance(chars, w2, mod)
    try:
        first = a.pairwise_ml_distances(MDL)
        a.set_pattern_weights(w2)
        Da, ea = a.pairwise_ml_distances(MDL, want=WANT)
        Db, eb = b.pairwise_ml_distances(MDL, want=WANT)
        assert not np.array_equal(first, Da)
        assert np.array_equal(Da, Db) and all(np.array_equal(ea[k], eb[k]) for k in WANT)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("ns", [4, 20])
def test_non_integer_weights(ns):
    """The same bits from call to call; counts within 1e-13 of numpy's (another order of additions); the optimiser against the
    restatement run on the DEVICE's counts and starting values"""
    mod = synth_model(ns)
    n, P = (13, 300) if ns == 4 else (7, 270)
    chars = synth_chars(n, P, ns)
    w = 0.1 + 2.9 * ((np.arange(P) * 0.6180339887498949) % 1.0)
    inst = make_instance(chars, w, mod)
    try:
        D, extra = inst.pairwise_ml_distances(MDL, want=WANT)
        D2, e2 = inst.pairwise_ml_distances(MDL, want=WANT)
        assert np.array_equal(D, D2) and all(np.array_equal(extra[k], e2[k]) for k in WANT)
        G = mr.raw_counts(mr.states_of(chars, ns), w, ns)
        F = G / np.maximum(G.sum(axis=(1, 2), keepdims=True), 1e-300)
        nz = F > 0
        assert np.array_equal(extra["counts"] > 0, nz) and rel(extra["counts"][nz], F[nz]).max() < 1e-13
        for x, (j, k) in enumerate(mr.pair_list(n)):
            d, lnl, it = mr.optimise_pair(extra["counts"][x], extra["initial"][j, k], mod, MDL)
            assert abs(D[j, k] - min(d, 2.0)) <= 1e-9 * min(d, 2.0) and it == extra["iterations"][x], (j, k)
    finally:
        inst.close()


# starting values passed in ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_initial_distances_argument(ns):
    mod = synth_model(ns)
    n, P = (13, 300) if ns == 4 else (7, 270)
    chars = synth_chars(n, P, ns)
    inst = make_instance(chars, np.ones(P), mod)
    try:
        D, extra = inst.pairwise_ml_distances(MDL, want=WANT)
        D2, e2 = inst.pairwise_ml_distances(MDL, initial=extra["initial"], want=WANT)
        assert np.array_equal(D, D2) and all(np.array_equal(extra[k], e2[k]) for k in WANT)
        moved = extra["initial"] * (1.0 + 1e-6)
        D3 = inst.pairwise_ml_distances(MDL, initial=moved)
        iu = np.triu_indices(n, 1)
        ok = (extra["initial"][iu] > 0) & (extra["initial"][iu] < 1.9) & (extra["iterations"] > 0)
        assert ok.any() and np.any(D3[iu][ok] != D[iu][ok])   # the argument is used
    finally:
        inst.close()


# sharded instances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,shards", [(4, 2), (4, 3), (20, 2), (20, 3)])
def test_sharded_instances(ns, shards):
    mod = synth_model(ns)
    n, P = (13, 302) if ns == 4 else (7, 271)
    chars = synth_chars(n, P, ns)
    w = 1.0 + (np.arange(P) % 3)
    one = make_instance(chars, w, mod)
    grp = make_instance(chars, w, mod, devices=[0] * shards, force_sharded=True)
    try:
        ranges = grp.shard_ranges()
        # a boundary inside a step of four patterns (4 states; 20-state shards start on whole fragment tiles by construction)
        assert len(ranges) == shards and (ns == 20 or any(lo % 4 for (_, lo, _) in ranges[1:])), ranges
        D, extra = one.pairwise_ml_distances(MDL, want=WANT)
        Dg, eg = grp.pairwise_ml_distances(MDL, want=WANT)
        assert np.array_equal(D, Dg) and all(np.array_equal(extra[k], eg[k]) for k in WANT)
        grp.set_pairwise_work_space(1)
        assert np.array_equal(grp.pairwise_ml_distances(MDL), D)
    finally:
        one.close(); grp.close()


# nothing else moves -----------------------------------------------------------------------------------------------------------------
def _fresh_answer(t, ot, ns):
    mod = mr.Model(ot.m.pi, ot.m.e_val, ot.m.r_e_vect, ot.m.l_e_vect, ot.m.l_min, ot.m.l_max)
    tv = np.stack([v for v in ot.tip_vec])
    inst = capi.Instance(ot.n, 2 * ot.n, ns, ot.P, 2 * ot.n, 1)
    try:
        inst.set_pattern_weights(ot.wght)
        inst.set_state_frequencies(mod.pi); inst.set_eigen_decomposition(mod.U, mod.V, mod.R)
        inst.set_phyml_options(mod.l_min, mod.l_max, 1.0, 1)
        for k in range(ot.n):
            inst.set_tip_partials(k, tv[k])
        return inst.pairwise_ml_distances(MDL)
    finally:
        inst.close()


@pytest.mark.parametrize("ns,P", [(4, 300), (20, 90)])
def test_nothing_else_moves(ns, P):
    t, ot, tree, st = synthetic_pair(13, P, ns, 4, seed=9, ambiguous_every=5)
    try:
        t.Set_Both_Sides(True)
        lnl = t.Lk(None)
        b5, b7 = t.Lk(5), t.Lk(7)
        out0, w0 = t.inst.site_outputs(), t.inst.numerical_warning()
        D = t.ML_Dist(MDL)
        assert np.array_equal(D, t.inst.pairwise_ml_distances(MDL))   # the host layer and the ABI call: the same bits
        assert np.array_equal(D, _fresh_answer(t, ot, ns))           # ... and the four rate classes of the tree play no part
        out1, w1 = t.inst.site_outputs(), t.inst.numerical_warning()
        assert w0 == w1 and all(np.array_equal(x, y) for x, y in zip(out0, out1))
        assert t.Lk(5) == b5 and t.Lk(7) == b7 and t.Lk(None) == lnl
        # behind a long queue: the traversal queued and not launched stays queued, the answer is the same
        t.Update_All_Partial_Lk()
        assert np.array_equal(t.ML_Dist(MDL), D)
        assert t.Lk(None) == lnl
    finally:
        t.close()


def test_with_virtual_buffers():
    """26 taxa: the whole-tree traversal leaves tip x tip results virtual, and nothing has to be stored for this call"""
    t, ot, tree, st = synthetic_pair(26, 150, 4, 4, seed=6, ambiguous_every=6)
    try:
        t.Set_Both_Sides(True)
        lnl = t.Lk(None)
        now = t.inst.virtual_stats()
        assert now[0] > 0
        D = t.ML_Dist(MDL)
        assert t.inst.virtual_stats() == now
        assert np.array_equal(D, _fresh_answer(t, ot, 4))
        assert t.Lk(None) == lnl
    finally:
        t.close()


def test_with_a_resident_evaluator_serving():
    """A chain of dLk calls served by the resident workgroups, the call in the middle of it"""
    t, ot, tree, st = synthetic_pair(14, 382, 4, 4, seed=23, ambiguous_every=17)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        D = t.ML_Dist(MDL)
        assert np.array_equal(D, _fresh_answer(t, ot, 4))
        e = 3
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        first = [t.dLk(0.003 * (i + 1), e)[1] for i in range(6)]
        assert t.inst.resident_stats(0)[0] > 0
        assert np.array_equal(t.ML_Dist(MDL), D)
        again = [t.dLk(0.003 * (i + 1), e)[1] for i in range(6)]
        assert first == again
        t.Set_Use_Eigen_Lr(False)
    finally:
        t.close()


# errors, profile ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_profile(golden):
    mod = synth_model(4)
    chars = synth_chars(5, 40, 4)
    inst = make_instance(chars, np.ones(40), mod)
    try:
        D = inst.pairwise_ml_distances(MDL)
        for kw in (dict(eigen_index=1), dict(eigen_index=-1), dict(frequencies_index=1), dict(frequencies_index=-1)):
            with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
                inst.pairwise_ml_distances(MDL, **kw)
        for bad in (0.0, -1e-3):
            with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
                inst.pairwise_ml_distances(bad)
        assert np.array_equal(inst.pairwise_ml_distances(MDL), D)   # the errors left nothing behind
        inst.profile(1)
        inst.profile_read_pairwise()
        inst.pairwise_ml_distances(MDL)
        cms, oms, calls = inst.profile_read_pairwise()
        assert calls == 1 and cms > 0 and oms > 0
        assert inst.profile_read_pairwise() == (0.0, 0.0, 0)
        inst.profile(0)
    finally:
        inst.close()
    cls = capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True)
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            cls.pairwise_ml_distances(MDL)
    finally:
        cls.close()
    from gpu_common import device_tree_from_golden
    t, ot = device_tree_from_golden(golden("nucleic_gtr_g4"), use_m4mod=True, arith=2)
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            t.inst.pairwise_ml_distances(MDL)
        with pytest.raises(capi.PhyhipError, match="generic-loop"):
            t.ML_Dist(MDL)
    finally:
        t.close()
