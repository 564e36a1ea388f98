"""Triple_Dist on the device (phyhip_optimise_triples, phyml_amd/csrc/phyhip_triple.hip) against the real reference's records
(tests/golden/triple_<case>.npz, tests/golden/make_triple.py), against tests/triple_ref.py over the CPU oracle, and against the chain
the host layer drives through the entry points that were there before (LkTree.Triple_Dist).

A candidate's second and third search start from lengths the first has found, and a spline root is only held to a few ulps of the
sums -- so no search is compared from the INPUT lengths on: search i is replayed on the CPU from the lengths the DEVICE held in front
of it (the inputs, then the device's own earlier outputs), and tests/test_gpu_brlen.py's single-search rules apply unchanged.
B_lnl / B_dlnl = P * 2^-52 * sum |terms| over the per-pattern lnL / dlnL terms (what two orders of adding the same terms can differ
by), the largest over the replayed search's probes.  Counts and statuses are exact.  l is exact where the path's best_l is the start or
a length of the two walks in factors of 1.2; a spline root lies within 8 x root_spread.  lnL lies within B_lnl of the oracle's dLk at
the device's l (the start itself: lkBegin, to the bits).  lkBegin lies within B_lnl of the oracle's Lk(e).  The kept vectors are the
oracle's update_partial at the device's final lengths, bit for bit."""
import os

import numpy as np
import pytest

import brlen_ref
import orc  # noqa: F401  (checker)
import phyg
import triple_ref
from gpu_common import assert_device_state_is_the_oracles, device_tree_from_golden, synthetic_pair
from phyml_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("nucleic_gtr_g4", "nucleic_gtr_g4_inv", "proteic_lg_g4")
SCALES = (1.0, 0.05, 20.0)


def _golden(name):
    return phyg.load(os.path.join(ROOT, "tests", "golden", name + ".phyg"))


def _candidate(t, a, factor=1.0, lengths=None):
    """((outer vectors), flags, (lengths)) of node a as Update_Partial_Lk / Lk resolve them on the host layer's tree"""
    nd = t.node(a).contents
    x, fl, ln = [], 0, []
    for i in range(3):
        b = nd.b[i].contents
        if b.left.contents.num == a:
            fl |= capi.triple_node_is_left(i)
            x.append(b.p_lk_tip_idx if b.rght.contents.tax else b.p_lk_rght_idx)
        else:
            x.append(b.p_lk_left_idx)
        ln.append(min(b.l * factor, 90.0))
    return tuple(x), fl, tuple(ln) if lengths is None else tuple(lengths)


def _edges(t, a):
    return [t.node(a).contents.b[i].contents.num for i in range(3)]


def _bounds(ot, r):
    b_lnl = b_dlnl = 0.0
    for lc in {r.l} | {p[0] for p in (r.probes if ot.P <= 64 else r.probes[-2:])}:
        _, x, y = ot.dlk_terms(lc)
        b_lnl = max(b_lnl, ot.P * 2.0 ** -52 * float(np.abs(x).sum()))
        b_dlnl = max(b_dlnl, ot.P * 2.0 ** -52 * float(np.abs(y).sum()))
    return b_lnl, b_dlnl


def _tied_lengths(r, l_start, lk_begin, b_lnl):
    """Where a walk crosses a stretch on which lnL moves by less than the sums' own bound (saturated trees: the slow category has
    clamped at l_min and the others carry no slope), `c_lnL > best_lnL` is decided by the order of the sum.  Both sides evaluate the
    same lengths; each device lnL lies within B_lnl of the oracle's, so the length the device calls best has an oracle lnL within
    2 B_lnl of the oracle's best.  Returns those lengths -- empty unless the replay itself took a best-so-far decision inside
    B_lnl (a record without one is held to the bits)."""
    if not any(k == "best" and m <= b_lnl for k, m in r.decisions):
        return set()
    tied = {p[0] for p in r.probes[1:] if abs(p[1] - r.lnL) <= 2.0 * b_lnl}      # (the first probe's lnL is never compared)
    return tied | ({l_start} if abs(lk_begin - r.lnL) <= 2.0 * b_lnl else set())


def _staged(ot, a, cand, res, what, iter_max=brlen_ref.BRENT_IT_MAX, ties=False):
    """the device's record of one candidate against the CPU replay of each search from the lengths the device held in front of it;
    the oracle tree is put back as it was.  ties: see _tied_lengths (the deep saturated trees only)."""
    e = triple_ref.edges_of(ot, a)
    l0 = [float(ot.len[x]) for x in e]
    held = list(cand[2])
    replays = []
    try:
        for i in range(3):
            if res.status[i] < 0:
                assert i > 0 and (res.status[i - 1] >= 3 or res.status[i - 1] < 0), (what, a, i, tuple(res.status))
                assert res.evaluations[i] == 0
                continue
            triple_ref.restore(ot, e, held)
            ot.update_partial(e[i], a)
            s = triple_ref.br_len_opt(ot, e[i], iter_max)
            r = s.result
            replays.append(s)
            b_lnl, b_dlnl = _bounds(ot, r)
            assert (res.evaluations[i], res.status[i]) == (r.evaluations, s.status), (what, a, i, tuple(res.evaluations), tuple(res.status), r.evaluations, s.status)
            assert abs(res.lkBegin[i] - s.lk_begin) <= b_lnl, (what, a, i, res.lkBegin[i], s.lk_begin, b_lnl)
            tied = _tied_lengths(r, held[i], s.lk_begin, b_lnl) if ties and r.best_from != "spline" and res.length[i] != r.l else set()
            if tied:
                assert res.length[i] in tied, (what, a, i, res.length[i].hex(), r.l.hex(), sorted(tied))
            elif r.best_from != "spline":
                assert res.length[i] == r.l, (what, a, i, res.length[i].hex(), r.l.hex())
            else:
                spread = brlen_ref.root_spread(r.spline, b_lnl, b_dlnl)
                assert abs(res.length[i] - r.l) <= 8.0 * spread, (what, a, i, res.length[i], r.l, spread)
            if i == 2 or res.status[i + 1] < 0:   # c_lnL as Triple_Dist leaves it: the last search's best_lnL (the oracle still holds its products)
                if r.best_from == "start" and res.length[i] == r.l:
                    assert res.lnL == res.lkBegin[i], (what, a, i)
                else:
                    assert abs(res.lnL - ot.dlk(res.length[i])[1]) <= b_lnl, (what, a, i, res.lnL, ot.dlk(res.length[i])[1], b_lnl)
            held[i] = res.length[i]
    finally:
        triple_ref.restore(ot, e, l0)
        for x in e:
            ot.update_partial(x, a)
    return replays


def _kept_vectors(t, ot, a, res, what):
    """the three kept vectors against the oracle's update_partial at the device's final lengths"""
    e = triple_ref.edges_of(ot, a)
    l0 = [float(ot.len[x]) for x in e]
    w = ot.wght > 0
    try:
        triple_ref.restore(ot, e, list(res.length))
        for i in range(3):
            ot.update_partial(e[i], a)
            side = 0 if a == ot.el[e[i]] else 1
            v, s = t.inst.triple_partials(i)
            assert np.array_equal(v[w], ot.plk[(e[i], side)][w]), (what, a, i)
            assert np.array_equal(s[w], ot.scale[(e[i], side)][w]), (what, a, i)
    finally:
        triple_ref.restore(ot, e, l0)
        for x in e:
            ot.update_partial(x, a)


def _prepare(t, ot):
    t.Set_Both_Sides(True)
    t.Lk(None)
    ot.lk(None, both_sides=True)


# ---- the reference's records, the CPU replay, the kept vectors and the chain on the three cases ------------------------------------
@pytest.fixture(scope="module", params=CASES)
def case(request):
    name = request.param
    d = _golden(name)
    t, ot = device_tree_from_golden(d)
    _prepare(t, ot)
    yield name, d, t, ot
    t.close()


def test_against_the_reference(case):
    """all internal nodes of a case at one scaling in ONE call: the statuses and the total of the evaluations -- as the growth of
    tree->n_tot_bl_opt, a function of the counts and statuses, which is what the reference records -- are the reference's at every
    kept record (lengths and c_lnL: the staged comparison below, which no propagated length blurs)"""
    name, d, t, ot = case
    f = np.load(os.path.join(ROOT, "tests", "golden", "triple_" + name + ".npz"))
    rows = range(len(f["node"]))
    assert {float(x) for x in f["scale"]} == set(SCALES) and len(rows) >= 3 * (ot.n - 2) * 9 // 10
    cands = [_candidate(t, int(f["node"][i]), float(f["scale"][i])) for i in rows]
    assert all(c[2] == tuple(float(x) for x in f["l_in"][i]) for i, c in zip(rows, cands))
    res = t.inst.optimise_triples(cands, iter_max=int(f["iter_max"][0]), tol=float(f["tol"][0]))   # every record of the case: ONE call
    for i, r in zip(rows, res):
        what = (name, int(f["node"][i]), float(f["scale"][i]))
        assert tuple(r.status) == tuple(int(x) for x in f["status"][i]), what
        n_tot = sum(ev - 1 + (1 if st in (1, 2, 7) else 0) for ev, st in zip(r.evaluations, r.status) if st >= 0 and ev > 0)
        assert n_tot == int(f["n_tot"][i]), what + (tuple(r.evaluations), int(f["n_tot"][i]))
        assert tuple(r.evaluations) == tuple(int(x) for x in f["evaluations"][i]), what   # (the restatement's split of that total)


@pytest.mark.parametrize("scale", SCALES)
def test_staged_against_the_cpu_replay_and_kept_vectors(case, scale):
    name, d, t, ot = case
    nodes = list(range(ot.n, 2 * ot.n - 2))
    cands = [_candidate(t, a, scale) for a in nodes]
    keep = len(nodes) // 2
    res = t.inst.optimise_triples(cands, keep=keep)
    assert t.inst.numerical_warning() == res[-1].warning == 0
    for a, c, r in zip(nodes, cands, res):
        _staged(ot, a, c, r, (name, scale))
    _kept_vectors(t, ot, nodes[keep], res[keep], (name, scale))


def test_against_the_host_driven_chain(case):
    """Triple_Dist through the host layer's Update_Partial_Lk / Br_Len_Opt -- the entry points that were there before -- at the same
    nodes: equal counts and statuses, equal lengths wherever the path's best_l is not a spline root, and the scan leaves the tree alone"""
    name, d, t, ot = case
    nodes = list(range(ot.n, 2 * ot.n - 2))[::3]
    res = t.inst.optimise_triples([_candidate(t, a) for a in nodes])
    before = t.n_tot_bl_opt
    l_scan, lnl_scan, st_scan = t.Triple_Dist_Scan(nodes)
    grown = t.n_tot_bl_opt - before
    assert [tuple(x) for x in l_scan] == [tuple(r.length) for r in res] and list(lnl_scan) == [r.lnL for r in res] and not st_scan.any()
    assert grown == sum(ev - 1 + (1 if st in (1, 2) else 0) for r in res for ev, st in zip(r.evaluations, r.status))
    assert_device_state_is_the_oracles(t, ot, what="around Triple_Dist_Scan")
    for a, r in zip(nodes, res):
        e = _edges(t, a)
        l0 = [float(d["edge_len"][x]) for x in e]
        # the chain search by search (the C function below makes exactly these calls)
        t.Update_PMat_At_Given_Edge(e[1]); t.Update_PMat_At_Given_Edge(e[2])
        chain = []
        for i in range(3):
            t.Update_Partial_Lk(e[i], a)
            chain.append(t.Br_Len_Opt(e[i], force_host_chain=True))
            assert not t.on_device
        for x, l in zip(e, l0):
            t.edge(x).contents.l = l
            t.Update_PMat_At_Given_Edge(x)
        lens, lnl, n_tot = t.Triple_Dist(a)
        assert lens == tuple(c[0] for c in chain) and lnl == chain[2][1], (name, a)
        assert n_tot == sum(ev - 1 + (1 if st in (1, 2) else 0) for ev, st in zip(r.evaluations, r.status)), (name, a)
        exact = True
        replays = _staged(ot, a, _candidate(t, a, lengths=l0), r, (name, "chain"))
        for i in range(3):
            assert chain[i][3:] == (r.evaluations[i], r.status[i]), (name, a, i, chain[i], tuple(r.evaluations), tuple(r.status))
            # from equal lengths in front of it, a search whose best_l is no spline root finds equal lengths on both routes
            replay = replays[i].result
            if exact and replay.best_from != "spline":
                assert chain[i][0] == r.length[i], (name, a, i, chain[i][0].hex(), r.length[i].hex())
            else:
                exact = False
        for x, l in zip(e, l0):
            t.edge(x).contents.l = l
            t.Update_PMat_At_Given_Edge(x)
        for x in e:
            t.Update_Partial_Lk(x, a)
    t.Lk(None)


def test_a_candidates_bits_depend_on_the_candidate_alone(case):
    name, d, t, ot = case
    nodes = list(range(ot.n, 2 * ot.n - 2))
    a = nodes[len(nodes) // 3]
    mine = _candidate(t, a, 20.0)
    alone = t.inst.optimise_triples([mine])[0].as_tuple()
    lst = [_candidate(t, nodes[k % len(nodes)], SCALES[k % 3]) for k in range(40)]
    lst[3] = lst[31] = mine
    whole = [r.as_tuple() for r in t.inst.optimise_triples(lst)]
    assert whole[3] == whole[31] == alone
    pe = (ot.P + 1) // 2 * 2
    fixed = (3 * (ot.P * ot.m.ncatg * ot.m.ns * 8 + pe * 4) + 255) // 256 * 256
    per = (3 * ot.m.ncatg * ot.m.ns ** 2 + ot.P * ot.m.ncatg * ot.m.ns) * 8 + pe * 4 + 136
    assert capi.triple_chunk_candidates(ot.P, ot.m.ncatg, ot.m.ns, fixed + 7 * per) == 7
    t.inst.set_triple_work_space(fixed + 7 * per)     # 40 candidates in chunks of 7: six chunks
    try:
        t.inst.profile(1)
        chunked = [r.as_tuple() for r in t.inst.optimise_triples(lst, keep=31)]
        ms, calls, evals = t.inst.profile_read_triples()
        t.inst.profile(0)
    finally:
        t.inst.set_triple_work_space(0)
    assert chunked == whole
    assert calls == 1 and ms > 0.0 and evals == sum(sum(r[4]) for r in whole)
    _kept_vectors(t, ot, a, t.inst.optimise_triples(lst, keep=31)[31], (name, "kept in a later chunk"))


# ---- geometry: W = workgroup threads, R = rounds of the search kept in registers ------------------------------------------------------
def _geometry():
    out = []
    for ns in (4, 20):
        w, r = capi.TRIPLE_THREADS[ns], capi.TRIPLE_KEEP[ns]
        for c in (1, 4, 8):
            cp = 1 << (c - 1).bit_length()
            # the search's lanes are (pattern, category): P * CP around W, and one P past the last register-kept round; the joins'
            # lanes are patterns: P around W
            for p in sorted({1, w // cp - 1, w // cp, w // cp + 1, r * w // cp + 1} | ({w - 1, w, w + 1} if c == 1 else set())):
                if p >= 1:
                    out.append((ns, c, p))
        # category counts that are no power of two: CP > C, triple_fetch's padded lanes c0 >= C read category 0 and dlk_lane masks them
        for c in (3, 5, 7):
            cp = 1 << (c - 1).bit_length()
            out.extend((ns, c, p) for p in sorted({1, w // cp, w // cp + 1}))
    return out


def _check_synthetic(t, ot, nodes, what, scales=SCALES, keep_at=0, ties=False):
    """returns the records [(scale, node, TripleResult.as_tuple())] and the exponents of the kept vectors per scale"""
    _prepare(t, ot)
    records, kept_exponents = [], []
    for scale in scales:
        cands = [_candidate(t, a, scale) for a in nodes]
        res = t.inst.optimise_triples(cands, keep=keep_at)
        for a, c, r in zip(nodes, cands, res):
            _staged(ot, a, c, r, (what, scale), ties=ties)
            records.append((scale, a, r.as_tuple()))
        _kept_vectors(t, ot, nodes[keep_at], res[keep_at], (what, scale))
        kept_exponents.append([t.inst.triple_partials(i)[1] for i in range(3)])
    return records, kept_exponents


@pytest.mark.parametrize("ns,c,p", _geometry())
def test_geometry(ns, c, p):
    t, ot, tree, st = synthetic_pair(6, p, ns, c, seed=100 + p % 17 + c)
    try:
        _check_synthetic(t, ot, (6, 9), (ns, c, p), keep_at=1)
    finally:
        t.close()


# ---- operand kinds and the tail's branches -----------------------------------------------------------------------------------------
def _rotated_pair(n, P, ns, C, seed):
    """synthetic_pair with every internal node's neighbour list rotated by its number: trees built from the root down have the node on
    the LEFT of its second and third edge everywhere; rotated, every edge position meets both orientations"""
    from gpu_common import synthetic_oracle
    from phyml_amd import lktree
    ot, tree, st, tv, wg = synthetic_oracle(n, P, ns, C, seed, ambiguous_every=11)
    nv = -np.ones((2 * n - 2, 3), np.int32); nb = -np.ones((2 * n - 2, 3), np.int32)
    for k, lst in enumerate(ot.adj):
        rot = lst[k % 3:] + lst[:k % 3] if len(lst) == 3 else lst
        for i, (v, b) in enumerate(rot):
            nv[k, i], nb[k, i] = v, b
    ot.set_adjacency(nv, nb)
    m = ot.m
    t = lktree.LkTree(n, tree.edge_left, tree.edge_rght, tree.edge_len, P, ns, C, node_v=nv, node_b=nb, host_pmat=True)
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)
    t.Make_Tree_For_Lk(wg)
    t.set_tips(tip_partials=tv)
    return t, ot


def test_each_operand_as_a_tip_and_both_values_of_each_flag():
    """over the internal nodes of a seven-taxon tree each of the three operands is a tip somewhere and each flag takes both values
    (asserted, not assumed); some tip patterns are ambiguous, some all-ones"""
    for ns, seed in ((4, 7), (20, 9)):
        t, ot = _rotated_pair(7, 130, ns, 4, seed)
        try:
            nodes = list(range(7, 12))
            cands = [_candidate(t, a) for a in nodes]
            tips = {i for x, fl, ln in cands for i in range(3) if x[i] < 7}
            flags = {(i, (fl >> i) & 1) for x, fl, ln in cands for i in range(3)}
            assert tips == {0, 1, 2} and flags == {(i, v) for i in range(3) for v in (0, 1)}, (tips, sorted(flags))
            _check_synthetic(t, ot, nodes, ("tips", ns), keep_at=2)
        finally:
            t.close()


def _own_and_inherited(ot, a):
    """whether some vector towards node a adds an exponent of its own, and whether some inherits one from its children"""
    own = inherited = False
    for e in triple_ref.edges_of(ot, a):
        side = 0 if a == ot.el[e] else 1
        kids = [ot.scale[k] for k in ot.op_for(e, a)[1] if k in ot.scale]
        below = sum(kids) if kids else 0
        inherited |= bool(np.any(below != 0))
        own |= bool(np.any(ot.scale[(e, side)] != below))
    return own, inherited


@pytest.mark.parametrize("name,nodes", [("nucleic_zero_w", (54, 60, 77, 105)), ("synth_nt_300x40", (300, 371, 450, 597)),
                                        ("nucleic_gtr_g4_inv", (54, 71, 105)), ("synth_aa_90x24", (90, 97, 98))])
def test_zero_weights_scale_exponents_and_invariant_sites(name, nodes):
    """bootstrap-like zero-weight patterns; a deep tree whose vectors carry inherited exponents and whose joins add their own, at
    both state counts (20 states: the join's second pass applies 2^256 -- other code than the 4-state registers); +I"""
    d = _golden(name)
    t, ot = device_tree_from_golden(d)
    try:
        _check_synthetic(t, ot, nodes, name, keep_at=1)
        if name in ("synth_nt_300x40", "synth_aa_90x24"):
            own = inherited = False
            for a in nodes:
                own_a, inherited_a = _own_and_inherited(ot, a)
                own, inherited = own or own_a, inherited or inherited_a
                if name == "synth_aa_90x24":
                    assert own_a and inherited_a, a      # at 20 states every one of the three nodes has both
            assert own and inherited
        if name == "nucleic_zero_w":
            assert np.any(ot.wght == 0)
    finally:
        t.close()


def test_near_zero_and_l_max_starts_and_iter_max():
    d = _golden("nucleic_gtr_g4")
    t, ot = device_tree_from_golden(d)
    try:
        _prepare(t, ot)
        a = 70
        x, fl, ln = _candidate(t, a)
        for lens in ((1e-9, ln[1], ln[2]), (ln[0], ot.m.l_max, ln[2]), (ln[0], ln[1], 2.0 * ot.m.l_max), (1e-9, 1e-9, 1e-9)):
            r = t.inst.optimise_triples([(x, fl, lens)])[0]
            _staged(ot, a, (x, fl, lens), r, ("starts", lens))
        # iterMax = 1: the first spline step is the first and last iteration -- status 5, where the reference stops the program: the
        # candidate ends there, its later searches are not reached, and a neighbour in the same call runs to its end
        lens = (ln[0] * 20.0, ln[1], ln[2])
        r, other = t.inst.optimise_triples([(x, fl, lens), _candidate(t, 71)], iter_max=1, keep=0)
        assert r.status[0] == 5 and tuple(r.status[1:]) == (-1, -1) and tuple(r.evaluations[1:]) == (0, 0) and r.evaluations[0] >= 3
        assert tuple(r.length[1:]) == lens[1:]
        _staged(ot, a, (x, fl, lens), r, "iterMax", iter_max=1)
        assert other.status[0] >= 0
        with pytest.raises(capi.PhyhipError) as ei:       # nothing is kept of a candidate that stopped
            t.inst.triple_partials(0)
        assert ei.value.code == capi.ERROR_OUT_OF_RANGE
        # the host layer's Triple_Dist stops there too: the exit handler runs with the reference's words and the two later edges are
        # not searched (the reference's program ends at that line)
        e = _edges(t, a)
        for b, l in zip(e, lens):
            t.edge(b).contents.l = l
        t.s_opt.brent_it_max = 1
        before = t.n_tot_bl_opt
        try:
            with pytest.raises(capi.PhyhipError, match="Too many iterations in edge length optimization routine"):
                t.Triple_Dist(a)
        finally:
            t.s_opt.brent_it_max = capi.BRENT_IT_MAX
        assert t.tree.contents.bl_opt_status == 5 and t.n_tot_bl_opt - before == r.evaluations[0] - 1
        assert [t.edge(b).contents.l for b in e[1:]] == list(lens[1:])
    finally:
        t.close()


@pytest.mark.parametrize("ns,P", [(4, 40), (20, 24)])
def test_without_lk_scaling(ns, P):
    """apply_lk_scaling = 0 on a deep tree with long branches: partials far below 2^-256 and no exponent anywhere -- not in the oracle's
    vectors, not among the kept ones, f = 0 in the tail; every 13th internal node at the three scalings"""
    t, ot, tree, st = synthetic_pair(120, P, ns, 4, seed=5, lmin=1.0, lmax=3.0, apply_scaling=0)
    try:
        nodes = list(range(ot.n, 2 * ot.n - 2))[::13]
        records, kept_exponents = _check_synthetic(t, ot, nodes, ("apply_lk_scaling = 0", ns), keep_at=3, ties=True)
        assert ot.apply_scaling == 0 and not any(np.any(s) for s in ot.scale.values())
        assert min(float(p[p > 0].min()) for p in ot.plk.values()) < 2.0 ** -256      # ... where scaling would have stepped in
        assert len(records) == 3 * len(nodes) and len(nodes) == 10
        for scale, a, (length, lnl, dlnl, lkb, evals, status, warning) in records:
            assert all(s in (0, 1, 2) for s in status) and warning == 0 and np.isfinite(lnl), (ns, scale, a, status, warning, lnl)
        assert not any(np.any(s) for per_scale in kept_exponents for s in per_scale)
        assert t.inst.numerical_warning() == 0
    finally:
        t.close()


def test_invariant_sites_at_twenty_states_with_scaled_constant_patterns():
    """+I at 20 states on a deep tree: planted constant columns, and branches long enough that constant patterns carry a nonzero
    exponent on every edge of the chosen nodes (asserted on the oracle) -- Invariant_Lk's scaled branch inside the probes"""
    t, ot, tree, st = synthetic_pair(90, 24, 20, 4, seed=5, lmin=4.0, lmax=8.0, pinvar=0.2, constant_every=4)
    try:
        nodes = (95, 97, 98)
        _prepare(t, ot)
        const = ot.invar >= 0
        assert ot.m.invar_model == 1 and ot.m.pinvar == 0.2 and 4 <= int(const.sum()) < ot.P
        for a in nodes:
            for e in triple_ref.edges_of(ot, a):
                ot.lk(e)
                assert np.any(ot.fact_sum_scale[const] != 0) and np.any(ot.fact_sum_scale[const] == 0), (a, e)
        _check_synthetic(t, ot, nodes, "+I at 20 states", keep_at=1, ties=True)
    finally:
        t.close()


def _outer_key(ot, a, e):
    """the oracle's key of the vector node a reads across its edge e: the side of e away from a"""
    return (e, 1 if a == ot.el[e] else 0)


@pytest.mark.parametrize("name,a,other", [("nucleic_gtr_g4", 58, 70), ("proteic_lg_g4", 54, 62)])
def test_small_floor_raises_the_candidates_own_warning(name, a, other):
    """The outer vectors of edge positions 0 and 1 of a node with three internal neighbours rewritten (x 1e-200 at patterns 1::7, on
    the device and in the oracle; a fresh tree, closed afterwards): those patterns are floored at SMALL in every evaluation of the
    node's three searches.  The oracle's warning is asserted first; the record's warning is the candidate's own, and the instance's
    flag is the LAST candidate's (include/phyhip.h)."""
    d = _golden(name)
    t, ot = device_tree_from_golden(d)
    try:
        _prepare(t, ot)
        e = triple_ref.edges_of(ot, a)
        mine, clean = _candidate(t, a), _candidate(t, other)
        assert all(x >= ot.n for x in mine[0]) and other not in [v for v, _ in ot.adj[a]]
        for i in (0, 1):
            key = _outer_key(ot, a, e[i])
            assert t.side_buffer(*key) == mine[0][i]
            ot.plk[key][1::7] *= 1e-200
            t.inst.set_partials(mine[0][i], ot.plk[key])
        assert t.inst.numerical_warning() == 0
        for node, want in ((a, 1), (other, 0)):          # the oracle first: Lk(b) on each of the node's edges
            for b in triple_ref.edges_of(ot, node):
                ot.update_partial(b, node)
                ot.lk(b)
                assert ot.numerical_warning == want, (name, node, b)
        res = t.inst.optimise_triples([mine, clean, mine], keep=0)
        assert [r.warning for r in res] == [1, 0, 1] and t.inst.numerical_warning() == 1
        for node, c, r in zip((a, other, a), (mine, clean, mine), res):
            replays = _staged(ot, node, c, r, (name, "SMALL floor"))
            assert all(s.status == 0 for s in replays) or node != a, (name, [s.status for s in replays])
        assert res[0].as_tuple() == res[2].as_tuple()
        assert res[0].lkBegin[0] < float(d["lnL"][0]) - 600.0 * len(range(1, ot.P, 7))     # log(DBL_MIN) = -708 per floored pattern
        _kept_vectors(t, ot, a, res[0], (name, "SMALL floor"))
        res = t.inst.optimise_triples([mine, clean])
        assert [r.warning for r in res] == [1, 0] and t.inst.numerical_warning() == 0
    finally:
        t.close()


# ---- a candidate that stops on real sums ----------------------------------------------------------------------------------------
def _first_search(ot, a, lens, pos=0):
    """triple_ref's search of edge position pos of node a from `lens`, the edges before it left as they are; the oracle tree is put back"""
    e = triple_ref.edges_of(ot, a)
    l0 = [float(ot.len[x]) for x in e]
    try:
        triple_ref.restore(ot, e, lens)
        ot.update_partial(e[pos], a)
        return triple_ref.br_len_opt(ot, e[pos])
    finally:
        triple_ref.restore(ot, e, l0)
        for x in e:
            ot.update_partial(x, a)


@pytest.mark.parametrize("name,a,start", [("nucleic_gtr_g4", 70, 1e308), ("nucleic_gtr_g4", 70, float("inf")), ("proteic_lg_g4", 57, 1e308)])
def test_a_candidate_that_stops_with_no_root_of_the_spline(name, a, start):
    """A start of 1e308 / +inf at edge position 0: the derivative is negative at l_max, the upper walk keeps v = the unclamped start,
    the cubic's coefficients overflow and u / v falls below 0.9 -- status 3, decided on infinities.  The candidate stops there: best_l
    so far, the two later searches not reached, nothing kept; its neighbours in the call are what they are alone.  The single-edge
    call and the host layer's two routes stop at the same count."""
    d = _golden(name)
    t, ot = device_tree_from_golden(d)
    try:
        _prepare(t, ot)
        x, fl, ln = _candidate(t, a)
        lens = (start, ln[1], ln[2])
        ref = _first_search(ot, a, lens)
        assert ref.status == brlen_ref.NO_ROOT and ref.result.best_from != "spline" and ref.result.evaluations >= 30, (name, ref.status)
        before, after = _candidate(t, a - 1, 20.0), _candidate(t, a + 1, 0.05)
        whole = t.inst.optimise_triples([before, (x, fl, lens), after], keep=2)
        r = whole[1]
        assert tuple(r.status) == (3, -1, -1) and tuple(r.evaluations) == (ref.result.evaluations, 0, 0), (tuple(r.status), tuple(r.evaluations))
        assert r.length[0] == ref.result.l and tuple(r.length[1:]) == tuple(lens[1:])
        _staged(ot, a, (x, fl, lens), r, (name, "status 3"))
        _kept_vectors(t, ot, a + 1, whole[2], (name, "kept beside a stopped candidate"))
        whole = [w.as_tuple() for w in whole]
        for c, got, node in ((before, whole[0], a - 1), (after, whole[2], a + 1)):
            alone = t.inst.optimise_triples([c])[0]
            assert alone.as_tuple() == got and got[5][2] in (0, 1, 2), (name, node, alone.as_tuple(), got)
            _staged(ot, node, c, alone, (name, "beside a stopped candidate"))
        t.inst.optimise_triples([before, (x, fl, lens), after], keep=1)
        with pytest.raises(capi.PhyhipError) as ei:       # nothing is kept of a candidate that stopped
            t.inst.triple_partials(0)
        assert ei.value.code == capi.ERROR_OUT_OF_RANGE
        # phyhip_optimise_edge_length from the same start on the same edge (the tree's other lengths are the candidate's)
        e = _edges(t, a)
        l0 = float(d["edge_len"][e[0]])
        t.edge(e[0]).contents.l = start
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        lkb = t.Lk(e[0])
        t.Set_Update_Eigen_Lr(False)
        single = t.inst.optimise_edge_length(start, lkb)
        assert single[3:] == (r.evaluations[0], 3) and single[0] == r.length[0]
        t.Set_Use_Eigen_Lr(False)
        # the host layer: Br_Len_Opt on either route and Triple_Dist stop with the status's words at the same count
        for route in (dict(force_host_chain=True), dict(force_device=True)):
            grown = t.n_tot_bl_opt
            with pytest.raises(capi.PhyhipError, match="no acceptable root of the spline"):
                t.Br_Len_Opt(e[0], l=start, **route)
            tr = t.tree.contents
            assert (tr.bl_opt_evaluations, tr.bl_opt_status) == (r.evaluations[0], 3) and t.on_device == ("force_device" in route)
            assert t.n_tot_bl_opt - grown == ref.result.n_tot == r.evaluations[0] - 1
            assert t.edge(e[0]).contents.l == r.length[0]          # best_l so far; the matrix is not rebuilt
        t.edge(e[0]).contents.l = start
        grown = t.n_tot_bl_opt
        with pytest.raises(capi.PhyhipError, match="no acceptable root of the spline"):
            t.Triple_Dist(a)
        assert t.tree.contents.bl_opt_status == 3 and t.n_tot_bl_opt - grown == r.evaluations[0] - 1
        assert [t.edge(b).contents.l for b in e] == [r.length[0], ln[1], ln[2]]
        t.edge(e[0]).contents.l = l0
        t.Update_PMat_At_Given_Edge(e[0])
    finally:
        t.close()


@pytest.mark.parametrize("start", [float("-inf"), 0.0, -1.0])
def test_starts_at_and_below_zero(start):
    """-inf, 0.0 and -1.0 at edge positions 0 and 1 of nucleic_gtr_g4's node 70: at position 1 the first probe (clamped to l_min)
    already has a negative derivative and the next length leaves [l_min, l_max] -- status 1 after one evaluation, l_out the UNCLAMPED
    start; at position 0 the walk goes up from l_min (73 evaluations on the CPU).  The device and the chain are held to the replay."""
    d = _golden("nucleic_gtr_g4")
    t, ot = device_tree_from_golden(d)
    try:
        _prepare(t, ot)
        a = 70
        x, fl, ln = _candidate(t, a)
        e = _edges(t, a)
        for pos in (0, 1):
            lens = tuple(start if i == pos else ln[i] for i in range(3))
            ref = _first_search(ot, a, lens, pos) if pos == 0 else None
            r = t.inst.optimise_triples([(x, fl, lens)], keep=0)[0]
            replays = _staged(ot, a, (x, fl, lens), r, ("start", start, pos))
            assert all(s in (0, 1, 2) for s in r.status), tuple(r.status)
            if pos == 1:
                assert (r.status[1], r.evaluations[1]) == (1, 1) and r.length[1] == start and replays[1].result.l == start
            else:
                assert (r.status[0], r.evaluations[0]) == (ref.status, ref.result.evaluations) and r.evaluations[0] >= 60
            _kept_vectors(t, ot, a, r, ("start", start, pos))
            # the chain: the host layer's Triple_Dist from the same lengths
            for b, l in zip(e, lens):
                t.edge(b).contents.l = l
            lens_chain, lnl, n_tot = t.Triple_Dist(a)
            assert n_tot == sum(ev - 1 + (1 if st in (1, 2) else 0) for ev, st in zip(r.evaluations, r.status)), (start, pos, n_tot)
            assert lens_chain[pos] == r.length[pos] or replays[pos].result.best_from == "spline"
            if pos == 1:
                assert lens_chain[1] == start
            for b in e:
                t.edge(b).contents.l = float(d["edge_len"][b])
                t.Update_PMat_At_Given_Edge(b)
            for b in e:
                t.Update_Partial_Lk(b, a)
    finally:
        t.close()


# ---- the documented maximum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [4, 20])
def test_the_documented_maximum_of_patterns(ns):
    """capi.TRIPLE_MAX_PATTERNS patterns, 8 categories: one candidate at scale 1.0 (the bounds from the last two probes, as above 64
    patterns everywhere), and the chunk bound for one candidate at this size"""
    assert capi.TRIPLE_MAX_PATTERNS == 16384
    t, ot, tree, st = synthetic_pair(6, 16384, ns, 8, seed=3)
    try:
        _check_synthetic(t, ot, (7,), ("maximum", ns), scales=(1.0,))
        pe = (ot.P + 1) // 2 * 2
        fixed = (3 * (ot.P * ot.m.ncatg * ot.m.ns * 8 + pe * 4) + 255) // 256 * 256
        per = (3 * ot.m.ncatg * ot.m.ns ** 2 + ot.P * ot.m.ncatg * ot.m.ns) * 8 + pe * 4 + 136
        assert capi.triple_chunk_candidates(ot.P, ot.m.ncatg, ot.m.ns, fixed + per) == 1
        assert capi.triple_chunk_candidates(ot.P, ot.m.ncatg, ot.m.ns, fixed + 2 * per) == 2
        cands = [_candidate(t, 7), _candidate(t, 8)]
        whole = [r.as_tuple() for r in t.inst.optimise_triples(cands)]
        t.inst.set_triple_work_space(fixed + per)          # one candidate per chunk
        try:
            assert [r.as_tuple() for r in t.inst.optimise_triples(cands, keep=1)] == whole
        finally:
            t.inst.set_triple_work_space(0)
    finally:
        t.close()


# ---- isolation -----------------------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing_of_the_instance():
    d = _golden("nucleic_gtr_g4")
    t, ot = device_tree_from_golden(d)
    try:
        _prepare(t, ot)
        e = 7
        l0 = float(d["edge_len"][e])
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        lkb = t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        dot = t.inst.get_dot_prod()
        mat = t.inst.get_transition_matrix(e)
        chain_before = [t.dLk(x, e) + (t.c_dlnL,) for x in (l0, l0 / 2, l0 * 3)]
        nodes = list(range(ot.n, 2 * ot.n - 2))
        res = t.inst.optimise_triples([_candidate(t, a, 20.0) for a in nodes], keep=5)
        assert all(r.status[2] in (0, 1, 2) for r in res)
        assert t.inst.numerical_warning() == 0
        assert np.array_equal(t.inst.get_dot_prod(), dot) and np.array_equal(t.inst.get_transition_matrix(e), mat)
        chain_after = [t.dLk(x, e) + (t.c_dlnL,) for x in (l0, l0 / 2, l0 * 3)]
        assert chain_before == chain_after
        t.Set_Use_Eigen_Lr(False)
        assert t.Lk(e) == lkb
        assert_device_state_is_the_oracles(t, ot, what="around phyhip_optimise_triples")
    finally:
        t.close()


def test_between_resident_served_evaluations():
    """tests/test_gpu_brlen.py::test_between_resident_served_evaluations with the new call in the middle: the dLk calls behind it are
    served resident again, none launched instead, and return the same doubles"""
    t, ot, tree, st = synthetic_pair(14, 382, 4, 4, seed=23, ambiguous_every=17)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        e = 3
        t.Set_Update_Eigen_Lr(True); t.Set_Use_Eigen_Lr(False)
        t.Lk(e)
        t.Set_Update_Eigen_Lr(False); t.Set_Use_Eigen_Lr(True)
        chain = lambda: [t.dLk(0.003 * (i + 1), e)[1] for i in range(6)]
        first = chain()
        served, _, _, instead = t.inst.resident_stats(0)
        assert served > 0
        res = t.inst.optimise_triples([_candidate(t, a, 20.0) for a in range(14, 26)])
        assert all(r.status[2] in (0, 1, 2) and min(r.evaluations) >= 1 for r in res)
        again = chain()
        assert first == again
        now = t.inst.resident_stats(0)
        assert now[0] == served + len(again) and now[3] == instead, (served, instead, now)
        t.Set_Use_Eigen_Lr(False)
    finally:
        t.close()


# ---- refusals and range errors: the documented code, nothing launched ---------------------------------------------------------------
@pytest.mark.parametrize("kw,p,c", [(dict(devices=[0, 0]), 300, 4), (dict(), capi.TRIPLE_MAX_PATTERNS + 1, 1), (dict(use_m4mod=True), 300, 4),
                                    (dict(), 40, 9)], ids=["sharded", "patterns", "generic-loop", "categories"])
def test_refusals_leave_the_per_candidate_route(kw, p, c):
    t, ot, tree, st = synthetic_pair(6, p, 4, c, seed=5, **kw)
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        t.inst.profile(1)
        with pytest.raises(capi.PhyhipError) as ei:
            t.inst.optimise_triples([_candidate(t, 7)])
        assert ei.value.code == capi.ERROR_NO_IMPLEMENTATION, (kw, p, c)
        assert t.inst.profile_read_triples()[1:] == (0, 0)
        t.inst.profile(0)
        with pytest.raises(capi.PhyhipError, match="phyhip_optimise_triples"):
            t.Triple_Dist_Scan([7])
        # ... and the per-candidate route serves the tree all the same
        lens, lnl, n_tot = t.Triple_Dist(7)
        assert n_tot >= 3 and np.isfinite(lnl)
    finally:
        t.close()


def _refused_with_nothing_launched(inst):
    inst.profile(1)
    with pytest.raises(capi.PhyhipError) as ei:
        inst.optimise_triples([((4, 5, 6), 0, (0.1, 0.1, 0.1))])
    assert ei.value.code == capi.ERROR_NO_IMPLEMENTATION and "phyhip_optimise_triples" in str(ei.value), str(ei.value)
    assert inst.profile_read_triples()[1:] == (0, 0)
    inst.profile(0)


def test_a_class_axis_instance_is_refused():
    """(also the only way to an instance of several eigen systems)"""
    inst = capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True)
    try:
        _refused_with_nothing_launched(inst)
    finally:
        inst.close()


def test_a_rank_is_refused():
    """a rank of phyhip_comm_init_rank holds only its own patterns: every probe would need every rank's sums"""
    rank = capi.Instance(4, 10, 4, 16, 5, 4)
    try:
        rank.comm_init_rank(1, 0, capi.comm_get_unique_id())
        _refused_with_nothing_launched(rank)
    finally:
        rank.close()


def test_range_errors_launch_nothing():
    t, ot, tree, st = synthetic_pair(6, 50, 4, 4, seed=5)
    try:
        _prepare(t, ot)
        t.inst.profile(1)
        x, fl, ln = [c for c in (_candidate(t, a) for a in range(6, 10)) if min(c[0]) < 6][0]
        assert t.inst.optimise_triples([]) == []
        nan = float("nan")
        i_tip = [i for i in range(3) if x[i] < 6][0]
        bad = [(dict(), [(x, fl, (nan, ln[1], ln[2]))], capi.ERROR_FLOATING_POINT),
               (dict(iter_max=0), [(x, fl, ln)], capi.ERROR_OUT_OF_RANGE), (dict(iter_max=capi.BRENT_IT_MAX + 1), [(x, fl, ln)], capi.ERROR_OUT_OF_RANGE),
               (dict(tol=0.0), [(x, fl, ln)], capi.ERROR_OUT_OF_RANGE), (dict(keep=1), [(x, fl, ln)], capi.ERROR_OUT_OF_RANGE),
               (dict(keep=-2), [(x, fl, ln)], capi.ERROR_OUT_OF_RANGE),
               (dict(), [((x[0], x[1], 10 ** 6), fl, ln)], capi.ERROR_OUT_OF_RANGE), (dict(), [((-1, x[1], x[2]), fl, ln)], capi.ERROR_OUT_OF_RANGE),
               (dict(), [(x, fl & ~capi.triple_node_is_left(i_tip), ln)], capi.ERROR_OUT_OF_RANGE)]
        for kw, cands, code in bad:
            with pytest.raises(capi.PhyhipError) as ei:
                t.inst.optimise_triples(cands, **kw)
            assert ei.value.code == code, (kw, cands)
        with pytest.raises(capi.PhyhipError) as ei:       # no call has kept anything yet
            t.inst.triple_partials(0)
        assert ei.value.code == capi.ERROR_OUT_OF_RANGE
        assert t.inst.profile_read_triples()[1:] == (0, 0)
        t.inst.optimise_triples([(x, fl, ln)], keep=0)
        for which in (-1, 3):
            with pytest.raises(capi.PhyhipError) as ei:
                t.inst.triple_partials(which)
            assert ei.value.code == capi.ERROR_OUT_OF_RANGE
        assert t.inst.profile_read_triples()[1] == 1
        t.inst.profile(0)
    finally:
        t.close()
