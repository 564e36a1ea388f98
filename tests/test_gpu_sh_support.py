"""phyhip_calculate_sh_support (Statistics_To_SH / Statistics_to_RELL on the device) against the restatement (tests/sh_ref.py, itself
held to the real reference by tests/test_sh_restatement.py) and against the reference's recorded supports
(tests/golden/sh_support_*.npz).

Bounds, all derived: a replicate's sums within siteCount x 2^-52 x sum |terms| of the exact (math.fsum) sum of the restatement's
draws with the same seed, the totals within patternCount x 2^-52 x sum |terms|; the acceptance and RELL flags equal to the
restatement's on every replicate whose margin exceeds 8 x that rounding bound (at most 0.1 % may fall short: the CPU test holds the
restatement to that at the same seed; expected none); SH and RELL of every recorded edge within 5 sqrt(2 p (1 - p) / R) + 2 / R of
the reference's recorded values (two independent Monte-Carlo estimates) plus that edge's undecided share.  Everything about determinism is bit for bit."""
import itertools

import numpy as np
import pytest

import sh_ref as sr
from gpu_common import synthetic_pair
from phyml_amd import capi

pytestmark = pytest.mark.gpu

R = sr.REPLICATES
SEED = sr.SEED


def make_instance(P, w, **kw):
    inst = capi.Instance(4, 10, 4, int(P), 5, 1, **kw)
    inst.set_pattern_weights(w)
    return inst


def load(inst, lks):
    for k in range(3):
        inst.set_support_site_lnl(k, lks[k])


def check_against(got, s, replicates):
    """A device answer (sh, rell, totals, {sums, accepted}) against a restatement dict of the same seed"""
    sh, rell, tot, extra = got
    sums, acc = extra["sums"], extra["accepted"]
    assert (np.abs(tot - s["totals_exact"]) <= s["totals_bound"]).all(), (tot, s["totals_exact"], s["totals_bound"])
    rows = s["exact_rows"]
    err = np.abs(sums[rows] - s["sums_exact"])
    assert (err <= s["sums_bound"][rows]).all(), (err.max(), s["sums_bound"][rows].min())
    assert (np.abs(sums - s["sums"]) <= 2 * s["sums_bound"]).all()   # (both lie within the bound of the exact sums)
    assert set(np.unique(acc)) <= {0, 1}
    cap = replicates // 1000
    assert (~s["decided"]).sum() <= cap and (~s["rell_decided"]).sum() <= cap
    d = s["decided"]
    assert np.array_equal(acc[d] == 1, s["accepted"][d]), np.where((acc == 1) != s["accepted"])[0][:10]
    dev_rell = (sums[:, 0] >= sums[:, 1]) & (sums[:, 0] >= sums[:, 2])
    d = s["rell_decided"]
    assert np.array_equal(dev_rell[d], s["rell_flags"][d])
    assert sh == acc.sum() / replicates and rell == dev_rell.sum() / replicates
    assert abs(sh - s["sh"]) <= (~s["decided"]).sum() / replicates and abs(rell - s["rell"]) <= (~s["rell_decided"]).sum() / replicates


# the alias table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nucleic", "proteic"])
def test_the_alias_table_is_the_restatements(name):
    """The library's table (built on its host side, read through the getter) equals the restatement's, which returns the reference's
    own indices (tests/test_sh_restatement.py): all four weight vectors, and rebuilt when the weights or the site count change"""
    fx = sr.fixture(name)
    sites = int(fx["init_len"][0])
    inst = make_instance(fx["alias_w"].shape[1], fx["alias_w"][0])
    try:
        for v in (0, 1, 2, 3, 0):
            inst.set_pattern_weights(fx["alias_w"][v])
            for n in (sites, sites + 1):
                prob, alias = inst.support_alias_table(n)
                want = sr.alias_table(fx["alias_w"][v], n)
                assert np.array_equal(prob, want[0]) and np.array_equal(alias, want[1]), (v, n)
    finally:
        inst.close()


# the recorded edges ------------------------------------------------------------------------------------------------------------------
ALL_EDGES = [(n, e) for n in ("nucleic", "proteic") for e in range(len(sr.fixture(n)["edges"]))]


@pytest.mark.parametrize("name,e", ALL_EDGES)
def test_the_references_supports(name, e):
    """Every recorded edge: SH and RELL with 10 000 replicates against the reference's own, within the Monte-Carlo bound plus the share
    of replicates the restatement, at the same seed, finds undecided (margin within 8 x the rounding bound): on those the flag may
    follow the order of additions, which is the reference's sequential one there and a wave's here.  That share is 0 on all but two
    edges.  Nucleic edge 89: 0.0075 for RELL.  Nucleic edge 103: its three vectors differ by at most 6.6e-14 (an internal branch of
    zero length), every replicate is undecided for RELL and the comparison is vacuous by this derivation (measured on an MI355X: 0.3875
    here, 0.7226 in the reference, 0.7302 in the sequential restatement); its SH, 0, is decided and compared like any other."""
    fx = sr.fixture(name)
    sites = int(fx["init_len"][0])
    s = sr.fixture_support(name, e)
    inst = make_instance(len(fx["wght"]), fx["wght"])
    try:
        load(inst, fx["lks"][e])
        sh, rell, tot = inst.sh_support(sites, R, SEED)
        for what, got, ref, und in (("SH", sh, fx["sh"][e], (~s["decided"]).sum() / R), ("RELL", rell, fx["rell"][e], (~s["rell_decided"]).sum() / R)):
            b = sr.mc_bound(got, ref, R) + und
            print(f"{name} edge {int(fx['edges'][e])} {what}: {got:.4f} reference {ref:.4f} bound {b:.4f} (undecided share {und:.4f})")
            assert abs(got - ref) <= b, (name, int(fx["edges"][e]), what, got, ref, b)
    finally:
        inst.close()


def test_undecided_shares_of_the_recorded_edges():
    """What the bound above adds, by the restatement alone: nothing on 45 of the 47 edges, and SH is decided everywhere"""
    und = {(n, e): ((~sr.fixture_support(n, e)["decided"]).sum(), (~sr.fixture_support(n, e)["rell_decided"]).sum()) for n, e in ALL_EDGES}
    assert all(v[0] == 0 for v in und.values())
    loose = {(n, int(sr.fixture(n)["edges"][e])): int(v[1]) for (n, e), v in und.items() if v[1]}
    assert set(loose) == {("nucleic", 89), ("nucleic", 103)} and loose[("nucleic", 103)] == R and loose[("nucleic", 89)] < R // 100, loose


@pytest.mark.parametrize("name,which", [(n, k) for n in ("nucleic", "proteic") for k in range(3)])
def test_recorded_edges_against_the_restatement(name, which):
    """Three recorded edges per fixture (lowest support, nearest one half, highest below one): sums, totals, flags, counts"""
    fx = sr.fixture(name)
    e = sr.picked_edges(name)[which]
    s = sr.fixture_support(name, e, exact_rows=np.arange(0, R, 97))
    inst = make_instance(len(fx["wght"]), fx["wght"])
    try:
        load(inst, fx["lks"][e])
        got = inst.sh_support(int(fx["init_len"][0]), R, SEED, want=("sums", "accepted"))
        check_against(got, s, R)
        assert np.array_equal(inst.support_alias_table(int(fx["init_len"][0]))[0], s["prob"])
    finally:
        inst.close()


# the smallest shapes at which the kernels can still go wrong -------------------------------------------------------------------------
@pytest.mark.parametrize("P,sites,reps,kind", sr.SHAPES)
def test_small_shapes(P, sites, reps, kind):
    lks, w, s = sr.shape_support(P, sites, reps, kind)
    inst = make_instance(P, w)
    try:
        load(inst, lks)
        got = inst.sh_support(sites, reps, SEED, want=("sums", "accepted"))
        check_against(got, s, reps)
        plain = inst.sh_support(sites, reps, SEED)
        assert plain[0] == got[0] and plain[1] == got[1] and np.array_equal(plain[2], got[2])
    finally:
        inst.close()


def test_identical_vectors_have_no_support():
    """delta = 0 can never exceed delta_local + 0.1; every replicate ties, so RELL is 1"""
    fx = sr.fixture("nucleic")
    l = fx["lks"][3][0]
    inst = make_instance(len(l), fx["wght"])
    try:
        load(inst, [l, l, l])
        sh, rell, tot, extra = inst.sh_support(int(fx["init_len"][0]), R, SEED, want=("sums", "accepted"))
        assert sh == 0.0 and rell == 1.0 and not extra["accepted"].any()
        assert tot[0] == tot[1] == tot[2] and np.array_equal(extra["sums"][:, 0], extra["sums"][:, 1]) and np.array_equal(extra["sums"][:, 0], extra["sums"][:, 2])
    finally:
        inst.close()


@pytest.mark.parametrize("order", list(itertools.permutations(range(3))))
def test_designed_triples(order):
    """One triple per ordering of the totals; across the replicates delta_local takes all six (asserted on the restatement)"""
    P, reps = 65, 3000
    lks = sr.designed_triple(P, order)
    s = sr.support(lks, np.ones(P), P, reps, SEED, exact_rows=np.arange(0, reps, 97))
    want_branch = {(0, 1, 2): 0, (0, 2, 1): 1, (1, 0, 2): 2, (1, 2, 0): 3, (2, 1, 0): 4, (2, 0, 1): 5}[order]
    assert s["delta_branch"] == want_branch and set(np.unique(s["local_branch"])) == set(range(6))
    inst = make_instance(P, np.ones(P))
    try:
        load(inst, lks)
        got = inst.sh_support(P, reps, SEED, want=("sums", "accepted"))
        check_against(got, s, reps)
        assert 0 < got[3]["accepted"].sum() < reps
    finally:
        inst.close()


# invariances, bit for bit ------------------------------------------------------------------------------------------------------------
def test_invariances():
    fx = sr.fixture("nucleic")
    sites = int(fx["init_len"][0])
    e = sr.picked_edges("nucleic")[1]
    inst = make_instance(len(fx["wght"]), fx["wght"])
    try:
        load(inst, fx["lks"][e])
        a = inst.sh_support(sites, R, SEED, want=("sums", "accepted"))
        b = inst.sh_support(sites, R, SEED, want=("sums", "accepted"))
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[3][k], b[3][k]) for k in a[3])
        # replicate r is the same whatever the replicate count (another grid, too)
        for r in (0, 1, 2, 63, 1000, 4999):
            c = inst.sh_support(sites, r + 1, SEED, want=("sums", "accepted"))
            assert np.array_equal(c[3]["sums"], a[3]["sums"][:r + 1]) and np.array_equal(c[3]["accepted"], a[3]["accepted"][:r + 1]), r
            assert np.array_equal(c[2], a[2])
        # another seed, in either word of the key: other sums
        for other in (SEED + 1, SEED ^ (1 << 40)):
            d = inst.sh_support(sites, 64, other, want=("sums",))
            assert not (d[3]["sums"] == a[3]["sums"][:64]).all(axis=1).any()
            assert np.array_equal(d[2], a[2])
        # re-uploading a slot and changing the weights and back: the same bits again
        inst.set_support_site_lnl(1, fx["lks"][e][1])
        inst.set_pattern_weights(np.ones(len(fx["wght"])))
        ones = inst.sh_support(sites, 100, SEED, want=("sums",))
        assert not np.array_equal(ones[2], a[2]) and not np.array_equal(ones[3]["sums"], a[3]["sums"][:100])   # another table, other totals
        inst.set_pattern_weights(fx["wght"])
        f = inst.sh_support(sites, R, SEED, want=("sums", "accepted"))
        assert f[:2] == a[:2] and np.array_equal(f[3]["sums"], a[3]["sums"])
    finally:
        inst.close()


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_sharded_instances_with_uploads(shards):
    fx = sr.fixture("proteic")
    sites = int(fx["init_len"][0])
    e = sr.picked_edges("proteic")[1]
    one = make_instance(len(fx["wght"]), fx["wght"])
    grp = make_instance(len(fx["wght"]), fx["wght"], devices=[0] * shards, force_sharded=True)
    try:
        assert len(grp.shard_ranges()) == shards
        load(one, fx["lks"][e]); load(grp, fx["lks"][e])
        a = one.sh_support(sites, 2000, SEED, want=("sums", "accepted"))
        b = grp.sh_support(sites, 2000, SEED, want=("sums", "accepted"))
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[3][k], b[3][k]) for k in a[3])
        pa, pb = one.support_alias_table(sites), grp.support_alias_table(sites)
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    finally:
        one.close(); grp.close()


# the NULL snapshot after a real Lk(b) -------------------------------------------------------------------------------------------------
def _snapshots(t, edges):
    """Lk(b) of three edges, each followed by the device-side snapshot; returns the three downloads of the same evaluations"""
    down = []
    for k, b in enumerate(edges):
        t.Lk(b)
        t.Set_Log_Lks_aLRT(k)
        down.append(t.inst.site_log_likelihoods())
    return np.stack(down)


@pytest.mark.parametrize("ns,P,shards", [(4, 300, 0), (20, 90, 0), (4, 302, 2), (4, 302, 3), (20, 271, 1)])
def test_null_snapshot_after_an_edge_evaluation(ns, P, shards):
    """Set_Log_Lks_aLRT after Lk(b) equals uploading the download of phyhip_get_site_log_likelihoods; partials, matrices, the last
    evaluation's outputs, the warning flag and the next evaluation stay what they were; a sharded tree gives the plain one's bits"""
    w = 1.0 + (np.arange(P) % 3)
    sites = int(w.sum())
    kw = dict(devices=[0] * shards, force_sharded=True) if shards else {}
    t, ot, tree, st = synthetic_pair(13, P, ns, 4, seed=9, ambiguous_every=5, wght=w, **kw)
    ref = make_instance(P, w)
    try:
        t.Set_Both_Sides(True)
        lnl = t.Lk(None)
        edges = (5, 7, 9)
        lk = [t.Lk(b) for b in edges]
        down = _snapshots(t, edges)
        out0, w0 = t.inst.site_outputs(), t.inst.numerical_warning()
        part0 = t.partials(5, 0)
        pm0 = t.inst.get_transition_matrix(5)
        assert t.tree.contents.init_len == sites
        sh = t.Statistics_To_SH(seed=SEED)
        rell = t.Statistics_to_RELL()
        got = t.inst.sh_support(sites, R, SEED, want=("sums", "accepted"))
        assert (sh, rell) == got[:2]                                    # the host layer and the ABI call: the same bits
        load(ref, down)
        want = ref.sh_support(sites, R, SEED, want=("sums", "accepted"))
        assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and all(np.array_equal(got[3][k], want[3][k]) for k in want[3])
        # totals against the evaluations' own scalars: the same patterns and weights, another order of additions
        assert np.allclose(got[2], lk, rtol=1e-12, atol=0)
        out1, w1 = t.inst.site_outputs(), t.inst.numerical_warning()
        assert w0 == w1 and all(np.array_equal(x, y) for x, y in zip(out0, out1))
        assert np.array_equal(t.partials(5, 0), part0) and np.array_equal(t.inst.get_transition_matrix(5), pm0)
        assert [t.Lk(b) for b in edges] == lk and t.Lk(None) == lnl
        # behind a queue: a NULL snapshot executes what is queued first, as the getter does
        t.Update_All_Partial_Lk()
        t.Set_Log_Lks_aLRT(0)
        t.Lk(edges[0])
        t.Set_Log_Lks_aLRT(0)
        assert t.Statistics_To_SH() == sh and t.Lk(None) == lnl
    finally:
        t.close(); ref.close()


def test_with_a_resident_evaluator_serving():
    """Edge evaluations of a small nucleotide tree are served by resident workgroups: the snapshot sees what they wrote"""
    P = 382
    t, ot, tree, st = synthetic_pair(14, P, 4, 4, seed=23, ambiguous_every=17)
    ref = make_instance(P, np.ones(P))
    try:
        t.Set_Both_Sides(True)
        t.Lk(None)
        for _ in range(4):
            down = _snapshots(t, (3, 4, 6))
        load(ref, down)
        assert t.inst.sh_support(P, 500, SEED, want=("sums",))[3]["sums"].tobytes() == ref.sh_support(P, 500, SEED, want=("sums",))[3]["sums"].tobytes()
    finally:
        t.close(); ref.close()


# errors, profile ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_profile(golden):
    P = 40
    lks = sr.designed_triple(P, (0, 1, 2))
    inst = make_instance(P, np.ones(P))
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
            inst.sh_support(P, 10, 1)                                   # no slot was ever set
        inst.set_support_site_lnl(0, lks[0]); inst.set_support_site_lnl(2, lks[2])
        with pytest.raises(capi.PhyhipError, match="slot 1 was never set"):
            inst.sh_support(P, 10, 1)
        for slot in (-1, 3):
            with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
                inst.set_support_site_lnl(slot, lks[0])
        inst.set_support_site_lnl(1, lks[1])
        good = inst.sh_support(P, 10, 1, want=("sums",))
        for sites, reps in ((0, 10), (-1, 10), (P, 0), (P, -3)):
            with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
                inst.sh_support(sites, reps, 1)
        with pytest.raises(capi.PhyhipError, match="phyhip error -5"):
            inst.support_alias_table(0)
        inst.set_pattern_weights(np.zeros(P))
        with pytest.raises(capi.PhyhipError, match="every pattern weight is zero"):
            inst.sh_support(P, 10, 1)
        w = np.ones(P); w[3] = -1.0
        inst.set_pattern_weights(w)
        with pytest.raises(capi.PhyhipError, match="negative"):
            inst.sh_support(P, 10, 1)
        inst.set_pattern_weights(np.ones(P))
        again = inst.sh_support(P, 10, 1, want=("sums",))             # the errors left nothing behind
        assert again[:2] == good[:2] and np.array_equal(again[3]["sums"], good[3]["sums"])
        inst.profile(1)
        inst.profile_read_support()
        inst.sh_support(P, 10, 1)
        ms, calls = inst.profile_read_support()
        assert calls == 1 and ms > 0
        assert inst.profile_read_support() == (0.0, 0)
        inst.profile(0)
    finally:
        inst.close()
    cls = capi.Instance(4, 10, 4, 16, 5, 4, class_axis=True)
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            cls.set_support_site_lnl(0, np.zeros(16))
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            cls.sh_support(16, 10, 1)
    finally:
        cls.close()
    from gpu_common import device_tree_from_golden
    t, ot = device_tree_from_golden(golden("nucleic_gtr_g4"), use_m4mod=True, arith=2)
    try:
        with pytest.raises(capi.PhyhipError, match="phyhip error -7"):
            t.inst.sh_support(10, 10, 1)
        with pytest.raises(capi.PhyhipError, match="generic-loop"):
            t.Set_Log_Lks_aLRT(0)
    finally:
        t.close()
