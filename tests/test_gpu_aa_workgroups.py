"""The 20-state traversal (phyml_amd/csrc/phyhip_aa.hpp: traverse_aa_kernel) with MORE THAN ONE consumer wave per workgroup: one
loader wave stages every operation's matrix tables into a four-item LDS ring, up to 15 consumer waves read them, and nothing but
s_ready and one s_done word per consumer keeps the loader from overwriting a slot that a slower consumer still reads.  The
consumer count is aa_nw = ceil(ntiles / compute units), so on a 256-CU device every alignment of at most 1024 patterns has ONE
consumer -- which is all the other per-buffer tests reach.  What can go wrong above that -- a slot overwritten too early, the
host's 8-table plan for in-step children, absent waves of the last workgroup, the block sum over present tiles only -- may move
one pattern of one "up" vector that neither the root sum nor a few edge evaluations read.

Check, through the C host layer: after Lk(NULL) EVERY internal partial vector and scale vector is np.array_equal to the oracle's
(tests/orc.py) on the patterns that carry weight, lnL is the oracle's to 1e-12, the per-site log-likelihoods to 1e-10 and
fact_sum_scale exactly -- at pattern counts derived from the device's compute-unit count, the smallest that give each geometry:

  shape  C  consumers  taxa  what
  a      4  2          12    plain list (10 operations post-order; both sides with every buffer stored), short launches
  a1     1  2          12    the same with 16 patterns per tile and cus + 1 tiles: the last workgroup holds ONE tile (an absent wave)
  b      4  3          24    list with in-step tip x tip children (the 8-table ring plan) and the all-stored run of the same instance
  c      4  3          60    174 operations both sides (more than 40 trips round the ring), rescaling in most buffers
  d      4  15         12    kAaMaxCons consumers, ragged last workgroup; list and short launches
  e1-e3  1-3  2        12    16, 8 and 4 patterns per tile (C = 3 leaves one MFMA block idle)
  f      4  2          12    every compute unit with a full workgroup (2 x cus tiles)
  g      4  2 / shard  12    two shards on one device, each with shape a's geometry

Ppad is a multiple of 16 patterns, so the tile count is a multiple of aa_cb(C) (4 for C = 3 and 4, 2 for C = 2): with TWO consumers
an absent wave (an odd tile count) exists for C = 1 only -- shapes a1 and e1 have one; a, e2, e3 and f cannot.  With 3 and 15
consumers (b, c, d) the last workgroup holds one and three tiles.  Every shape's last tile is ragged (P = tiles x patterns per tile - r).
"""
import collections
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc  # noqa: F401
from gpu_common import assert_device_state_is_the_oracles, device_compute_units, synthetic_oracle
from phyml_amd import lktree, replay
from replay_oracle import OracleReplayer

K_AA_MAX_CONS = 15  # kAaMaxCons, phyml_amd/csrc/phyhip_aa.hpp:66


def aa_cb(C):
    """MFMA blocks per pattern, phyml_amd/csrc/phyhip_kernels.hpp:247"""
    return 1 if C == 1 else (2 if C == 2 else 4)


def launch_geometry(P, C, cus):
    """build_instance's own lines, phyml_amd/csrc/phyhip.hip:209 (Ppad), :245-247 (ntiles, cus, aa_nw) and :261 (grid_aa):
    (tiles, consumer waves per workgroup, workgroups)"""
    Ppad = (P + 15) // 16 * 16
    ntiles = Ppad // (16 // aa_cb(C))
    aa_nw = min(K_AA_MAX_CONS, max(1, (ntiles + cus - 1) // cus))
    return ntiles, aa_nw, (ntiles + aa_nw - 1) // aa_nw


Shape = collections.namedtuple("Shape", "C nw taxa absent r zeros seed lmin lmax full shards", defaults=(0.02, 0.3, False, 1))
SHAPES = {
    "a": Shape(4, 2, 12, False, 1, True, 21),
    "a1": Shape(1, 2, 12, True, 5, False, 22),
    "b": Shape(4, 3, 24, True, 1, True, 23),
    "c": Shape(4, 3, 60, True, 2, False, 8, 0.05, 0.6),
    "d": Shape(4, 15, 12, True, 3, True, 25),
    "e1": Shape(1, 2, 12, True, 9, False, 26),
    "e2": Shape(2, 2, 12, False, 3, False, 27),
    "e3": Shape(3, 2, 12, False, 2, False, 28),
    "f": Shape(4, 2, 12, False, 1, False, 29, full=True),
    "g": Shape(4, 2, 12, False, 1, True, 30, shards=2),
}


def tile_count(s, cus):
    """The fewest tiles above (nw - 1) x cus that Ppad can produce (a multiple of aa_cb(C)) with / without a ragged last workgroup;
    full: nw x cus, every workgroup complete"""
    cb = aa_cb(s.C)
    if s.full:
        assert (s.nw * cus) % cb == 0
        return s.nw * cus
    for k in range(1, cus + 1):
        ntiles = (s.nw - 1) * cus + k
        if ntiles % cb == 0 and (ntiles % s.nw != 0) == s.absent:
            return ntiles
    raise AssertionError(f"no tile count with {s.nw} consumers on {cus} compute units for {s}")


def pattern_count(s, cus):
    """patterns of ONE instance (of one shard): the last tile lacks r patterns"""
    npw = 16 // aa_cb(s.C)
    assert 1 <= s.r < npw
    return npw * tile_count(s, cus) - s.r


def weights(P, zeros):
    w = 1.0 + (np.arange(P) % 3)
    if zeros:
        w[3::5] = 0.0
    return w


def make_oracle(name, cus):
    """(oracle tree, random tree, tip vectors, weights, patterns): nothing evaluated yet"""
    s = SHAPES[name]
    P = pattern_count(s, cus) * s.shards
    ot, tree, _, tv, wg = synthetic_oracle(s.taxa, P, 20, s.C, s.seed, s.lmin, s.lmax, wght=weights(P, s.zeros), ambiguous_every=7)
    return ot, tree, tv, wg, P


Ref = collections.namedtuple("Ref", "name s cus ot tree tv wg P lnl site fact post")


@functools.lru_cache(maxsize=None)
def reference(name, cus):
    """The oracle after Lk(NULL) on both sides: computed once per shape, read-only afterwards.  (The post-order buffers and the
    root edge's outputs are those of a post-order-only evaluation: the pre-order pass writes other buffers.)"""
    ot, tree, tv, wg, P = make_oracle(name, cus)
    lnl = ot.lk(None, both_sides=True)
    ops = []
    ot.post_order(ot.tip_root, ot.adj[ot.tip_root][0][0], ops=ops)
    post = [ot.op_for(e, d)[0] for (e, d) in ops]
    return Ref(name, SHAPES[name], cus, ot, tree, tv, wg, P, lnl, ot.c_lnL_sorted.copy(), ot.fact_sum_scale.copy(), post)


@functools.lru_cache(maxsize=None)
def compute_units():
    return device_compute_units()


def ref_of(name):
    """the shape's reference at this device's geometry, with the geometry asserted: the mirrored aa_nw is the target, the last
    workgroup is ragged where the shape says so, and the last tile is"""
    cus = compute_units()
    r = reference(name, cus)
    s = r.s
    P1 = r.P // s.shards
    assert P1 * s.shards == r.P
    ntiles, aa_nw, wgs = launch_geometry(P1, s.C, cus)
    print(f"shape {name}: {cus} compute units, {s.taxa} x {r.P} patterns, C = {s.C}: {ntiles} tiles, aa_nw = {aa_nw}, {wgs} workgroups, "
          f"last workgroup {ntiles - (wgs - 1) * aa_nw} tile(s)")
    assert ntiles == tile_count(s, cus)       # Ppad still yields the intended tile count
    assert aa_nw == s.nw, (aa_nw, s.nw)
    assert (ntiles % aa_nw != 0) == s.absent
    assert wgs > 1 and P1 % (16 // aa_cb(s.C)) != 0
    if name in ("a1", "e1"):
        assert ntiles == cus + 1                # one tile in the last workgroup
    return r


def device_tree(r, host_pmat=True, devices=None, force_sharded=False):
    m = r.ot.m
    t = lktree.LkTree(r.ot.n, r.tree.edge_left, r.tree.edge_rght, r.tree.edge_len, r.P, 20, r.s.C, host_pmat=host_pmat, devices=devices,
                      force_sharded=force_sharded)
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)
    t.Make_Tree_For_Lk(r.wg)
    t.set_tips(tip_partials=r.tv)
    return t


def where(r, got, exp):
    """the first pattern that differs as (pattern, tile, workgroup, consumer wave, tiles of that workgroup)"""
    bad = np.flatnonzero(np.any(np.asarray(got).reshape(r.P, -1) != np.asarray(exp).reshape(r.P, -1), axis=1) & (r.wg > 0))
    P1 = r.P // r.s.shards
    ntiles, nw, _ = launch_geometry(P1, r.s.C, r.cus)
    p = int(bad[0]) % P1
    tile = p // (16 // aa_cb(r.s.C))
    return dict(differing=len(bad), pattern=int(bad[0]), tile=tile, workgroup=tile // nw, wave=tile % nw,
                tiles_in_workgroup=min(nw, ntiles - tile // nw * nw))


def assert_buffers(t, r, keys, what):
    """every listed partial vector and scale vector, bit for bit, on the patterns with weight"""
    w = r.wg > 0
    for k in keys:
        got, sc = t.partials(*k), t.scale_factors(*k)
        assert np.array_equal(got[w], r.ot.plk[k][w]), (what, "partials", k, where(r, got, r.ot.plk[k]))
        assert np.array_equal(sc[w], r.ot.scale[k][w]), (what, "scale", k, where(r, sc, r.ot.scale[k]))


def assert_evaluation(t, r, both, what, repeat=False, kernel=None, virtual=None):
    """points 1-3 (and 5 with repeat) of what every shape asserts; returns lnL.  kernel: what the instance (under phyhip_profile)
    must name as the evaluation's launch -- asked before anything is read back: reading a virtual buffer is a launch of its own."""
    keys = list(r.ot.plk) if both else r.post
    assert len(keys) == (3 if both else 1) * (r.s.taxa - 2)
    w = r.wg > 0
    t.Set_Both_Sides(both)
    lnl = t.Lk(None)
    print(f"  {what}: lnL {lnl!r} oracle {r.lnl!r}, virtual {t.inst.virtual_stats()}")
    if kernel is not None:
        assert re.fullmatch(kernel, t.inst.profile_read_kernel()), (what, t.inst.profile_read_kernel())
    if virtual is not None:
        assert (t.inst.virtual_stats()[0] > 0) == virtual, (what, t.inst.virtual_stats())
    assert abs(lnl - r.lnl) <= 1e-12 * abs(r.lnl), (what, lnl, r.lnl)
    site, _, _, fact = t.inst.site_outputs()
    assert np.max(np.abs(site[w] - r.site[w])) < 1e-10, what
    assert np.array_equal(fact[w], r.fact[w]), what
    assert t.inst.numerical_warning() == 0
    assert_buffers(t, r, keys, what)
    if repeat:
        # three evaluations in a row of the unchanged tree (the second and third reuse the list cached in a device slot): the same
        # double each time, and the same buffers
        again = [t.Lk(None) for _ in range(3)]
        assert again == [lnl] * 3, (what, lnl, again)
        assert_buffers(t, r, keys, (what, "after three more"))
    return lnl


PLAIN = r"traverse_aa_kernel<%d, false, 0, false, false, 1, false>"
IN_STEP = r"traverse_aa_kernel<%d, false, 0, false, true, 1, false>"
ARGUMENTS = r"traverse_aa_kernel<%d, false, 0, true, false, 1, false>"


@pytest.mark.parametrize("both", [False, True], ids=["post_order", "both_sides"])
@pytest.mark.parametrize("name", ["a", "a1"])
def test_plain_list_with_two_consumers(name, both):
    r = ref_of(name)
    t = device_tree(r)
    try:
        t.inst.set_virtual_buffers(0)
        t.inst.profile(1)
        assert_evaluation(t, r, both, (name, both), repeat=(name == "a"), kernel=PLAIN % r.s.C)
        assert t.inst.virtual_stats() == (0, 0, 0, 0)
    finally:
        t.close()


def test_in_step_children_with_three_consumers():
    """shape b: the default run computes its tip x tip results inside the steps that read them (four tables per ring item, the
    host's plan of the 8-table ring); the companion stores every one -- the other instantiation.  Both are the oracle's, per buffer."""
    r = ref_of("b")
    t, t0 = device_tree(r), device_tree(r)
    try:
        t0.inst.set_virtual_buffers(0)
        for x in (t, t0):
            x.inst.profile(1)
            x.Set_Both_Sides(True)
        lnl, lnl0 = t.Lk(None), t0.Lk(None)
        assert lnl == lnl0
        assert t.inst.virtual_stats()[0] > 0 and t0.inst.virtual_stats()[0] == 0
        assert re.fullmatch(IN_STEP % 4, t.inst.profile_read_kernel()), t.inst.profile_read_kernel()
        assert re.fullmatch(PLAIN % 4, t0.inst.profile_read_kernel()), t0.inst.profile_read_kernel()
        assert assert_evaluation(t, r, True, "b in-step", repeat=True, kernel=IN_STEP % 4) == lnl
        assert assert_evaluation(t0, r, True, "b all stored", repeat=True, kernel=PLAIN % 4) == lnl
    finally:
        t.close(); t0.close()


def test_long_list_rescales_round_the_ring():
    """shape c: 174 operations both sides -- more than 40 trips round the four-item ring -- on a tree deep enough to rescale.  The
    inputs decide something: at least a third of the oracle's scale vectors hold a non-zero exponent and the root edge's sum reaches
    256."""
    r = ref_of("c")
    assert len(r.ot.plk) == 174
    rescaled = sum(int(np.any(sc != 0)) for sc in r.ot.scale.values())
    print(f"shape c: {rescaled} of {len(r.ot.scale)} scale vectors hold a non-zero exponent, fact_sum_scale up to {r.fact.max()}")
    assert 3 * rescaled >= len(r.ot.scale), rescaled
    assert r.fact.max() >= 256
    t = device_tree(r)
    try:
        assert_evaluation(t, r, True, "c", virtual=True)
    finally:
        t.close()


@pytest.mark.parametrize("name", ["d", "e1", "e2", "e3", "f"])
def test_list_both_sides(name):
    r = ref_of(name)
    t = device_tree(r)
    try:
        assert_evaluation(t, r, True, name, repeat=(name == "d"))
    finally:
        t.close()


def test_two_shards_with_two_consumers_each():
    """shape g: the pattern range split over two shards on one device, each shard an instance of shape a's geometry"""
    r = ref_of("g")
    t = device_tree(r, devices=[0, 0], force_sharded=True)
    try:
        rng = t.inst.shard_ranges()
        assert len(rng) == 2 and [x[2] for x in rng] == [r.P // 2] * 2
        assert_evaluation(t, r, True, "g")
    finally:
        t.close()


@pytest.mark.parametrize("host_pmat", [True, False], ids=["host_matrices", "device_matrices"])
@pytest.mark.parametrize("name", ["a", "d"])
def test_argument_form(name, host_pmat):
    """The short launches -- launched, because the resident evaluator takes instances of one consumer only (resident_aa_eligible:
    aa_nw == 1): the evaluation alone at three edges (the list instantiation with no operation), one and two updates + the
    evaluation with their records in the kernel arguments, then a seeded SPR / Br_Len_Opt call stream (one or two updates + the
    evaluation per candidate; device_matrices: the matrices rebuilt inside the launch) against the oracle call by call, and what
    the stream leaves in the tree's own buffers against the oracle's, bit for bit."""
    cus = compute_units()
    ref_of(name)                                     # (the geometry's assertions)
    ot, tree, tv, wg, P = make_oracle(name, cus)     # (an oracle of its own: the stream writes it)
    r = Ref(name, SHAPES[name], cus, ot, tree, tv, wg, P, None, None, None, None)
    t = device_tree(r, host_pmat=host_pmat)
    try:
        t.Set_Both_Sides(True)
        ref = ot.lk(None, both_sides=True)
        assert abs(t.Lk(None) - ref) <= 1e-12 * abs(ref)
        t.inst.profile(1)
        for e in (0, t.ne // 2, t.ne - 1):
            got, ref = t.Lk(e), ot.lk(e)
            print(f"  {name} Lk({e}): {got!r} oracle {ref!r} {t.inst.profile_read_kernel()}")
            assert abs(got - ref) <= 1e-12 * abs(ref), (e, got, ref)
            assert re.fullmatch(PLAIN % 4, t.inst.profile_read_kernel()), t.inst.profile_read_kernel()
        b = [e for e in range(ot.ne) if ot.el[e] >= ot.n and ot.er[e] >= ot.n][1]
        forms = []
        for n_up in (1, 2):
            for d in (int(ot.el[b]), int(ot.er[b]))[:n_up]:
                t.Update_Partial_Lk(b, d)
                ot.update_partial(b, d)
            got, ref = t.Lk(b), ot.lk(b)
            print(f"  {name} {n_up} update(s) + Lk({b}): {got!r} oracle {ref!r} {t.inst.profile_read_kernel()}")
            assert abs(got - ref) <= 1e-12 * abs(ref), (n_up, got, ref)
            forms.append(t.inst.profile_read_kernel())
        # (a short launch whose operations equal a list still cached in a device slot is served from that slot, as a list: the
        # host's choice, build_op_records -- every other one carries its records in the kernel arguments)
        assert all(re.fullmatch(ARGUMENTS % 4, f) or re.fullmatch(PLAIN % 4, f) for f in forms), forms
        assert any(re.fullmatch(ARGUMENTS % 4, f) for f in forms), forms
        assert_device_state_is_the_oracles(t, ot, what=(name, host_pmat, "short launches"))
        assert t.inst.resident_stats(1)[0] == 0
        tr = replay.make_trace(ot.n, tree.edge_left, tree.edge_rght, tree.edge_len, 30, seed=13, walk_every=3, opt_every=4, n_dlk=3)
        assert t.spare_p_lk_idx == replay.side_buffer_map(ot.n, tree.edge_left, tree.edge_rght)[1]
        got, got2 = t.Replay_Surface_Trace(tr)
        rep = OracleReplayer(ot)
        ref, ref2 = rep.run(tr)
        k = tr["kind"]
        lnl_calls = (k == replay.EDGE_LNL) | (k == replay.DLK)
        assert lnl_calls.sum() >= 30
        assert np.max(np.abs(got[lnl_calls] - ref[lnl_calls]) / np.abs(ref[lnl_calls])) < 1e-11
        dl = k == replay.DLK
        assert dl.any()
        assert np.max(np.abs(got2[dl] - ref2[dl]) / np.maximum(1.0, np.abs(ref2[dl]))) < 1e-8
        assert t.inst.resident_stats(1)[0] == 0      # nothing was served by resident workgroups
        assert_device_state_is_the_oracles(t, ot, {key: idx for idx, key in rep.key_of.items()}, (name, host_pmat))
    finally:
        t.close()
