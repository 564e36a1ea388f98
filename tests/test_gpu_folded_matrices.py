"""Device-built transition matrices on the routes a search takes: queued with phyhip_update_transition_matrices and FOLDED into
the evaluation that reads them (FlushPlan::fold_pm, TreeParams::n_fresh), where code of the evaluation kernels rebuilds them --
nt2_run's prologue (the launched short forms, the list form, the small resident evaluators with the exp table in LDS, the
large-grid resident kernel) and the 20-state resident rebuild on the matrix cores.  The standalone pmat_kernel / pmat20_kernel
launches are held to the oracle's bits elsewhere (tests/test_gpu_cases.py::test_device_built_matrices_at_every_category_count);
here every rebuilt matrix, every partial vector and scale vector the call wrote and the matrices it did not touch are compared
with the oracle's bit for bit, the returned lnL to 1e-12 (the bar of the host-matrix route at the same shapes), and every
case shows that the intended route ran.

Two families of edge lengths.  'phyml': PhyML's own clamps (l_min = 1e-8, l_max = 100), lengths over the whole range they let
through plus 0, a negative one and 1e-300 -- with the committed eigen systems exp()'s argument stays inside (-212, 0], so of
the rare branches of phyhip_exp_ref only |x| < 2^-54 is reached (through the near-zero first eigenvalue).  'wide': the clamps
opened (l_min = 0) so that ONE folded batch holds ordinary arguments next to every rare class -- zero, |x| < 2^-54, the
subnormal results of 512 <= |x| < 745, the underflow of 745 <= |x| < 1024 inside the same branch, and |x| >= 1024.  That is a
condition on the inputs, asserted on the CPU for every batch before anything is compared (_assert_rare_batch), and checked
without a device, together with the oracle's behaviour on such matrices, by test_the_plans_hold_every_exp_class_and_the_oracle_stays_finite.
(A single matrix cannot hold an argument below 2^-54 next to one beyond 512: 'wide' batches have at least two matrices.)"""
import re

import numpy as np
import pytest

import orc  # noqa: F401
from gpu_common import assert_device_state_is_the_oracles, synthetic_oracle, synthetic_pair

gpu = pytest.mark.gpu
WIDE = (0.0, 1.0e7)  # l_min, l_max of the 'wide' family


# ---- the inputs: plans of (matrices to rebuild, partial updates, evaluation edge), made on the CPU ---------------------------

def _exp_arguments(m, lens):
    """exp()'s arguments for a batch of edge lengths, as every matrix builder forms them (src/lk.c:2296-2300, src/models.c:275):
    [matrix, category, eigenvalue]"""
    ln = np.maximum(np.asarray(lens, dtype=np.float64), 0.0)[:, None] * m.gamma_rr[None, :]
    ln = ln * m.br_len_mult
    ln = np.where(ln < m.l_min, m.l_min, np.where(ln > m.l_max, m.l_max, ln))
    return m.e_val[None, None, :] * ln[:, :, None]


def _classes(x):
    a = np.abs(x)
    return {"zero": bool((x == 0.0).any()), "tiny": bool((a < 2.0 ** -54).any()), "ordinary": bool(((a >= 2.0 ** -54) & (a < 512.0)).any()),
            "subnormal": bool(((a >= 512.0) & (a < 745.0)).any()), "underflow": bool(((a >= 745.0) & (a < 1024.0)).any()),
            "far": bool((a >= 1024.0).any())}


def _assert_rare_batch(m, lens):
    cl = _classes(_exp_arguments(m, lens))
    assert all(cl.values()), (cl, lens)


def _lengths(m, rng, family, k, step):
    """k edge lengths of one batch"""
    if family == "phyml":
        lens = 10.0 ** rng.uniform(-9, 2.3, k)
        special = [0.0, -0.25, 1e-300]
        if k >= 4:
            lens[:3] = special
        else:
            lens[0] = special[step % 3]
        return [float(v) for v in rng.permutation(lens)]
    assert k >= 2
    amax = float(np.max(np.abs(m.e_val)) * np.max(m.gamma_rr))
    one = None  # ONE length whose matrix holds ordinary arguments, subnormal results, underflow and |x| >= 1024 side by side
    for X in rng.permutation(np.arange(1030.0, 4000.0, 7.0)):
        cl = _classes(_exp_arguments(m, [X / amax]))
        if cl["ordinary"] and cl["subnormal"] and cl["underflow"] and cl["far"]:
            one = X / amax
            break
    assert one is not None
    more = [lambda: 10.0 ** rng.uniform(-22, -18), lambda: rng.uniform(520, 740) / amax, lambda: rng.uniform(750, 1020) / amax,
            lambda: 10.0 ** rng.uniform(3.1, 5) / amax, lambda: 10.0 ** rng.uniform(-3, 0.5), lambda: 10.0 ** rng.uniform(-3, 0.5)]
    lens = [one, 0.0] + [more[i % len(more)]() for i in range(k - 2)]
    _assert_rare_batch(m, lens)
    return [float(v) for v in rng.permutation(lens)]


def _candidate(ot, rng, family, k, b, updates, step, taken=()):
    """Rebuild k matrices -- edge b's, which Lk(b) queues itself (the last of the batch), and k - 1 in front of it, the ones the
    partial updates read first -- update the sides of b at the nodes `updates`, evaluate at b."""
    read = []
    for d in updates:
        read += [be for (_, be) in ot.adj[d] if be != b and be not in read]
    rest = [int(e) for e in rng.permutation(ot.ne) if e != b and e not in read and e not in taken]
    lens = _lengths(ot.m, rng, family, k, step)
    return dict(b=int(b), updates=[int(d) for d in updates], pre=(read + rest)[:k - 1], pre_len=lens[:k - 1], b_len=lens[k - 1])


def _device_candidate(t, c):
    for e, l in zip(c["pre"] + [c["b"]], c["pre_len"] + [c["b_len"]]):
        t.edge(e).contents.l = l
    if c["pre"]:
        t.inst.update_transition_matrices(np.array(c["pre"], np.int32), np.array(c["pre_len"]))
    for d in c["updates"]:
        t.Update_Partial_Lk(c["b"], d)
    return t.Lk(c["b"])  # (Update_PMat_At_Given_Edge(b) queues the last matrix; the evaluation folds the batch)


def _oracle_candidate(ot, c):
    for e, l in zip(c["pre"], c["pre_len"]):
        ot.len[e] = l
        ot.update_pmat(e)
    ot.len[c["b"]] = c["b_len"]
    for d in c["updates"]:
        ot.update_partial(c["b"], d)
    v = ot.lk(c["b"])
    assert np.isfinite(v) and ot.numerical_warning == 0
    return v


def _set_family(ot, family, t=None):
    m = ot.m
    if family == "wide":
        m.l_min, m.l_max = WIDE
        if t is not None:
            t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)


def _internal_edges(ot):
    return [e for e in range(ot.ne) if ot.el[e] >= ot.n and ot.er[e] >= ot.n]


def _short_form_ks(C):
    """1, a full round of the prologue (MPR = 64 / (4 C) matrices), one more (a second round), 8 (the most a launch folds), 9
    (pmat_kernel in front: the control)"""
    mpr = 64 // (4 * C)
    return sorted({1, min(mpr, 8), min(mpr + 1, 8), 8, 9})


def _short_form_plan(ot, family, seed):
    """[(updates in the launch, k, candidate)]: every short form at every k"""
    rng = np.random.default_rng(seed)
    inner = _internal_edges(ot)
    plan = []
    for n_up in (0, 1, 2):
        for k in _short_form_ks(ot.m.ncatg):
            if family == "wide" and k < 2:
                continue
            b = inner[len(plan) % len(inner)]
            updates = [ot.el[b], ot.er[b]][:n_up]
            plan.append((n_up, k, _candidate(ot, rng, family, k, b, updates, len(plan))))
    return plan


def _list_plan(ot, family, seed):
    """two rounds of: 8 lengths change (pendant and internal edges), then the whole tree is traversed and evaluated"""
    rng = np.random.default_rng(seed)
    inner = _internal_edges(ot)
    pend = [e for e in range(ot.ne) if e not in inner]
    plan = []
    for step in range(2):
        idx = [int(e) for e in rng.permutation(pend)[:4]] + [int(e) for e in rng.permutation(inner)[:4]]
        plan.append((idx, _lengths(ot.m, rng, family, 8, step)))
    return plan


def _resident_plan(ot, family, seed, ks):
    """SPR-candidate shaped commands (src/spr.c:640-646: three matrices, one partial update, Lk(b)); k = 4 adds a matrix the command
    does not read.  No two of them rebuild the same matrix or write the same buffer, so what each one wrote is still there when
    the sequence is over (nothing is read back in between: a read-back sends the large-grid workgroups away)."""
    rng = np.random.default_rng(seed)
    taken, cands = set(), []
    for step, k in enumerate(ks):
        d = next(int(d) for d in rng.permutation(np.arange(ot.n, 2 * ot.n - 2)) if not any(be in taken for (_, be) in ot.adj[d]))
        b = ot.adj[d][int(rng.integers(3))][1]
        c = _candidate(ot, rng, family, k, b, [d], step, taken)
        taken |= {c["b"], *c["pre"]}
        cands.append(c)
    return cands


SHORT = [(P, C, f) for P in (17, 70) for C in (1, 2, 3, 4) for f in ("phyml", "wide")]
LIST = [(C, f) for C in (3, 4) for f in ("phyml", "wide")]
SMALL = [(P, C, f) for P in (382, 1500) for C in (3, 4) for f in ("phyml", "wide")]
LARGE = [(12, 5000, 4), (12, 7000, 3)]
AA = [(C, f) for C in (1, 2, 3, 4) for f in ("phyml", "wide")]


def test_the_plans_hold_every_exp_class_and_the_oracle_stays_finite():
    """No device: every plan the GPU tests below run is made (the 'wide' ones assert the rare-class condition batch by batch) and
    the oracle follows it -- with l_min = 0 and lengths from 0 to beyond exp()'s underflow orc.pmat_edge returns finite,
    row-normalised matrices (1e-100 floors; numpy's sum of a row of 20 is 1 within a few ulps) and every likelihood stays finite, without a
    numerical warning.  And what PhyML's own clamps let through, with the committed eigen systems: exp()'s argument never
    reaches -512, so the 'phyml' family exercises the ordinary branch and |x| < 2^-54 only."""
    def follow(ot, cands):
        for c in cands:
            _oracle_candidate(ot, c)
        assert np.isfinite(ot.pm).all() and ot.pm.min() > 0.0 and np.max(np.abs(ot.pm.sum(-1) - 1.0)) < 1e-14

    for ns in (4, 20):
        ot = synthetic_oracle(6, 3, ns, 4, seed=1)[0]
        x = _exp_arguments(ot.m, [0.0, 1e-300, 1e-9, 100.0, 1e3])
        cl = _classes(x)
        assert np.abs(x).max() < 512.0 and cl["tiny"] and cl["ordinary"] and not (cl["subnormal"] or cl["underflow"] or cl["far"])
    for P, C, family in SHORT:
        if P != 17:
            continue
        ot = synthetic_oracle(10, P, 4, C, seed=5 + C, ambiguous_every=7)[0]
        _set_family(ot, family)
        ot.lk(None, both_sides=True)
        plan = _short_form_plan(ot, family, 100 + C)
        assert {(u, k) for u, k, _ in plan} >= {(u, k) for u in (0, 1, 2) for k in (8, 9)}
        follow(ot, [c for _, _, c in plan])
    for C, family in LIST:
        ot = synthetic_oracle(24, 130, 4, C, seed=9 + C, ambiguous_every=11)[0]
        _set_family(ot, family)
        ot.lk(None, both_sides=True)
        for idx, lens in _list_plan(ot, family, 200 + C):
            for e, l in zip(idx, lens):
                ot.len[e] = l
                ot.update_pmat(e)
            assert np.isfinite(ot.lk(None, both_sides=True, refresh_pmat=False)) and ot.numerical_warning == 0
    for family in ("phyml", "wide"):
        for n, P, ns, C, ks in ((14, 382, 4, 3, (3, 4, 4, 3)), (14, 382, 4, 4, (3, 4, 4, 3)), (12, 300, 4, 4, (3, 4, 3)), (12, 300, 4, 3, (3, 4, 3)),
                                (16, 60, 20, 1, (3, 4, 4, 3)), (16, 60, 20, 2, (3, 4, 4, 3)), (16, 60, 20, 3, (3, 4, 4, 3)), (16, 60, 20, 4, (3, 4, 4, 3))):
            ot = synthetic_oracle(n, P, ns, C, seed=31 + C, ambiguous_every=13)[0]
            _set_family(ot, family)
            ot.lk(None, both_sides=True)
            follow(ot, _resident_plan(ot, family, 300 + C, ks))


# ---- nucleotides, launched ----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("P,C,family", SHORT)
def test_launched_short_forms_rebuild_the_oracles_matrices(P, C, family, monkeypatch):
    """traverse_nt2_kernel<C, G, false, ARGS>: the evaluation alone (ARGS = 3), one update + evaluation (1), two updates + evaluation
    (2), each with 1, MPR, MPR + 1 and 8 queued matrices folded into its prologue and with 9, which pmat_kernel rebuilds in front
    (the control: same assertions).  The route: under phyhip_profile the instance names the kernel form of its last traversal
    launch and counts the launches -- one per call.  The existing getters do NOT tell a folded batch from a pmat_kernel launch in
    front of the same traversal kernel (pmat_kernel is not among the profiled launches): that the batches of up to 8 are folded is
    the host's rule (plan_route: at most 8 matrices, at most 4 categories, a small grid), and the k = 8 / k = 9 pair straddles it."""
    monkeypatch.setenv("PHYHIP_RESIDENT", "0")
    t, ot, *_ = synthetic_pair(10, P, 4, C, seed=5 + C, host_pmat=False, ambiguous_every=7)
    worst = 0.0
    try:
        _set_family(ot, family, t)
        t.inst.set_virtual_buffers(0)  # (every buffer stored: the launches below hold exactly the operations queued here)
        t.Set_Both_Sides(True)
        ref = ot.lk(None, both_sides=True)
        assert abs(t.Lk(None) - ref) <= 1e-12 * abs(ref)
        assert_device_state_is_the_oracles(t, ot, what="whole tree")
        t.inst.profile(True)
        launches = t.inst.profile_read()[1]
        for n_up, k, c in _short_form_plan(ot, family, 100 + C):
            got, ref = _device_candidate(t, c), _oracle_candidate(ot, c)
            name, now = t.inst.profile_read_kernel(), t.inst.profile_read()[1]
            assert re.fullmatch(r"traverse_nt2_kernel<%d, \d, false, %d>" % (C, (3, 1, 2)[n_up]), name), (n_up, k, name)
            assert now == launches + 1, (n_up, k, now, launches)
            launches = now
            # the k rebuilt matrices and the others; the buffers the call wrote and the others; the scalar
            assert_device_state_is_the_oracles(t, ot, what=(n_up, k, c))
            assert abs(got - ref) <= 1e-12 * abs(ref), (n_up, k, got, ref)
            worst = max(worst, abs(got - ref) / abs(ref))
        assert t.inst.resident_stats(1)[0] == 0 and t.inst.numerical_warning() == 0
        print(f"short forms P={P} C={C} {family}: worst relative lnL difference {worst:.3g}")
    finally:
        t.close()


@gpu
@pytest.mark.parametrize("C,family", LIST)
def test_list_form_rebuilds_the_oracles_matrices(C, family, monkeypatch):
    """The list form with in-step children (24 taxa: a both-sides traversal of 66 operations, tip x tip results virtual) and 8
    folded matrices: 8 pendant and internal lengths change, then the whole tree is traversed and evaluated at the root edge.
    (Lk(NULL) itself queues ALL the tree's matrices in one call -- 45 here, and a call of 32 or more launches pmat_kernel at once
    -- so the traversal and the evaluation are issued as Lk(NULL) issues them, without its Update_All_PMat: the 8 are what is
    queued when the launch is made.)  The route: the instance names the list form with in-step children as the kernel of the
    launch, one launch per round."""
    monkeypatch.setenv("PHYHIP_RESIDENT", "0")
    t, ot, *_ = synthetic_pair(24, 130, 4, C, seed=9 + C, host_pmat=False, ambiguous_every=11)
    try:
        _set_family(ot, family, t)
        t.Set_Both_Sides(True)
        ref = ot.lk(None, both_sides=True)
        assert abs(t.Lk(None) - ref) <= 1e-12 * abs(ref)
        b = ot.root_edge()
        eb = t.edge(b).contents
        parent, child = eb.p_lk_left_idx, (eb.p_lk_tip_idx if eb.rght.contents.tax else eb.p_lk_rght_idx)
        t.inst.profile(True)
        launches = t.inst.profile_read()[1]
        for idx, lens in _list_plan(ot, family, 200 + C):
            for e, l in zip(idx, lens):
                t.edge(e).contents.l = l
                ot.len[e] = l
                ot.update_pmat(e)
            t.inst.update_transition_matrices(np.array(idx, np.int32), np.array(lens))
            # (storing the virtual buffers that were defined on the old matrices is a launch of its own, made by the call above)
            launches = t.inst.profile_read()[1]
            t.Update_All_Partial_Lk()
            got = t.inst.edge_lnl(parent, child, eb.Pij_rr_idx)
            ref = ot.lk(None, both_sides=True, refresh_pmat=False)
            name, now = t.inst.profile_read_kernel(), t.inst.profile_read()[1]
            assert re.fullmatch(r"traverse_nt2_kernel<%d, \d, false, 0, 2, true>" % C, name), name
            assert now == launches + 1, (now, launches)
            assert_device_state_is_the_oracles(t, ot, what=(idx, lens))
            assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)
            print(f"list form C={C} {family}: relative lnL difference {abs(got - ref) / abs(ref):.3g}")
        assert t.inst.numerical_warning() == 0
    finally:
        t.close()


# ---- resident workgroups ----------------------------------------------------------------------------------------------------------

def _resident_case(t, ot, family, seed, ks, which, resident=True):
    """Warm up -- Lk(b) at every edge: each queues ONE matrix (unchanged length) and folds it; the first stores what the whole-tree
    traversal left virtual, the next ones find the workgroups there -- then the candidates, back to back, nothing read in between;
    then the oracle follows, and scalars, matrices and buffers are compared.  which: the evaluator that must have served EVERY
    candidate (phyhip_get_resident_stats index)."""
    _set_family(ot, family, t)
    t.Set_Both_Sides(True)
    first = t.Lk(None)
    cands = _resident_plan(ot, family, seed, ks)
    warm = [t.Lk(e) for e in range(ot.ne)]
    got, served = [], []
    for c in cands:
        s0 = t.inst.resident_stats(which)[0]
        got.append(_device_candidate(t, c))
        served.append(t.inst.resident_stats(which)[0] - s0)
    stats = t.inst.resident_stats(which)
    ref = ot.lk(None, both_sides=True)
    assert abs(first - ref) <= 1e-12 * abs(ref)
    worst = 0.0
    for e, v in enumerate(warm):
        ref = ot.lk(e)
        assert abs(v - ref) <= 1e-12 * abs(ref), (e, v, ref)
    for c, v in zip(cands, got):
        ref = _oracle_candidate(ot, c)
        assert abs(v - ref) <= 1e-12 * abs(ref), (c, v, ref)
        worst = max(worst, abs(v - ref) / abs(ref))
    if resident:
        assert served == [1] * len(cands) and stats[2] == 0, (served, stats)
    else:
        assert stats[0] == 0, stats
    assert_device_state_is_the_oracles(t, ot, what=cands)
    assert t.inst.numerical_warning() == 0
    return worst


@gpu
@pytest.mark.parametrize("P,C,family", SMALL)
def test_small_resident_evaluators_rebuild_the_oracles_matrices(P, C, family, monkeypatch):
    """The short-launch resident evaluator (382 patterns: every workgroup polls the host; 1 500: workgroup 0 relays the commands),
    exp table in LDS: SPR-candidate commands with 3 and 4 folded matrices, every one of them served by the resident workgroups."""
    monkeypatch.setenv("PHYHIP_RESIDENT", "1")
    t, ot, *_ = synthetic_pair(14, P, 4, C, seed=31 + C, host_pmat=False, ambiguous_every=13)
    try:
        worst = _resident_case(t, ot, family, 300 + C, (3, 4, 4, 3), 1)
        print(f"small resident P={P} C={C} {family}: worst relative lnL difference {worst:.3g}")
    finally:
        t.close()


@gpu
@pytest.mark.parametrize("taxa,P,C", LARGE)
@pytest.mark.parametrize("family", ["phyml", "wide"])
def test_large_grid_resident_kernel_rebuilds_the_oracles_matrices(taxa, P, C, family, monkeypatch):
    """resident_big_kernel (5 000 patterns at 4 categories: two lanes per pattern; 7 000 at 3: one lane), where only a wave's first
    tile rebuilds the command's matrices: candidates with 3 and 4 folded matrices, every one served by the resident workgroups."""
    monkeypatch.setenv("PHYHIP_RESIDENT", "1")
    t, ot, *_ = synthetic_pair(taxa, P, 4, C, seed=31 + C, host_pmat=False, ambiguous_every=13)
    try:
        worst = _resident_case(t, ot, family, 300 + C, (3, 4, 3), 2)
        print(f"large-grid resident P={P} C={C} {family}: worst relative lnL difference {worst:.3g}")
    finally:
        t.close()


@gpu
@pytest.mark.parametrize("C,family", AA)
@pytest.mark.parametrize("resident", ["1", "0"])
def test_20_state_evaluators_rebuild_the_oracles_matrices(C, family, resident, monkeypatch):
    """20 states, 60 patterns: the resident form of traverse_aa_kernel rebuilds the queued matrices on the matrix cores -- candidates
    with 3 matrices, all read by the command, and with 4, one of which the command does not read (the spare item of the LDS ring)
    -- every one served by the resident workgroups; PHYHIP_RESIDENT=0: pmat20_kernel + a launch per call, the control (same
    inputs, same assertions, nothing served)."""
    monkeypatch.setenv("PHYHIP_RESIDENT", resident)
    t, ot, *_ = synthetic_pair(16, 60, 20, C, seed=31 + C, host_pmat=False, ambiguous_every=13)
    try:
        worst = _resident_case(t, ot, family, 300 + C, (3, 4, 4, 3), 1, resident == "1")
        print(f"20 states C={C} {family} resident={resident}: worst relative lnL difference {worst:.3g}")
    finally:
        t.close()
