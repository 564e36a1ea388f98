"""The nucleotide step's dependent chain (phyml_amd/csrc/phyhip_nt2.hpp, profiles/r09_nt_chain.md): the rescaling maximum is
exchanged between the lanes of a pattern in registers, a step's records are loaded and the next operation's matrices staged into
LDS one half-step before they are consumed.  What can go wrong is the exchanged maximum, and a record or a matrix piece consumed
one step off -- either shows in the partial vectors or the scale exponents of some internal buffer.

Check, through the C ABI: after Lk(NULL) EVERY internal partial vector and scale vector is np.array_equal to the oracle's
(tests/orc.py), and lnL equals the all-stored run of the same instance (set_virtual_buffers(0): lists without in-step children,
the other instantiation of every kernel).  GTR + Gamma4 on synth.random_tree / simulate_states:

  300 x 96       two lanes per pattern, list form (traverse_nt2_kernel<4, 2>); long list, even length
  301 x 96       the same with one operation more: odd length, padded by the host
  40 x 8 230     two wave shapes in one launch (traverse_nt2_mixed_kernel<4>): 256 full two-lane workgroups + a four-lane rest
  20 x 131 200   one lane per pattern (traverse_nt2_kernel<4, 1>): the smallest padded size above the two-lane range (2 048 waves)
  40 x 8 230 N   fully ambiguous columns in two sister tips and in their aunt: an in-step child that is all ones meets the
                 all-ones rule of the operation above it
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import orc
from gpu_common import synthetic_oracle
from phyml_amd import lktree, synth, workloads


def sisters_with_tip_aunt(ot):
    """(tip, tip, tip): two tips below one node and a tip that is the sister of that node"""
    for d in range(ot.n, len(ot.adj)):
        kids = [v for (v, _) in ot.adj[d] if v < ot.n]
        ups = [v for (v, _) in ot.adj[d] if v >= ot.n]
        if len(kids) == 2 and len(ups) == 1:
            aunts = [v for (v, _) in ot.adj[ups[0]] if v < ot.n]
            if aunts:
                return kids[0], kids[1], aunts[0]
    raise AssertionError("no cherry with a tip aunt in this tree")


def ambiguous_oracle(n_otu, P, seed):
    """synthetic_oracle's model, tree and states, with 'N' in every 5th column of two sister tips and every 10th of their aunt"""
    plain, tree, st, _, wg = synthetic_oracle(n_otu, P, 4, 4, seed)
    a, b, c = sisters_with_tip_aunt(plain)
    chars = synth.states_to_chars(st, 4).copy()
    chars[a, 0::5] = ord("N"); chars[b, 0::5] = ord("N"); chars[c, 0::10] = ord("N")
    m = plain.m
    tv, ds, amb = [], [], []
    for t in range(n_otu):
        v, s, x = orc.init_tip(m.datatype, chars[t])
        tv.append(v); ds.append(s); amb.append(x)
    ot = orc.OracleTree(m, n_otu, tree.edge_left, tree.edge_rght, tree.edge_len, wg, tv, ds, amb, apply_scaling=1, arith=1)
    return ot, tree, tv, wg


@functools.lru_cache(maxsize=None)
def reference(n_otu, P, seed, ambiguous):
    """(oracle tree after Lk(NULL), its lnL, random tree, tip vectors, weights): computed once per shape, read-only afterwards"""
    if ambiguous:
        ot, tree, tv, wg = ambiguous_oracle(n_otu, P, seed)
    else:
        ot, tree, _, tv, wg = synthetic_oracle(n_otu, P, 4, 4, seed)
    return ot, ot.lk(None), tree, tv, wg


def device_tree(ot, tree, tv, wg, P):
    m = ot.m
    t = lktree.LkTree(ot.n, tree.edge_left, tree.edge_rght, tree.edge_len, P, 4, 4, host_pmat=True)
    t.set_model(m.pi, m.gamma_rr, m.gamma_r_proba, m.e_val, m.r_e_vect, m.l_e_vect, m.l_min, m.l_max, 1.0, 1)
    t.Make_Tree_For_Lk(wg)
    t.set_tips(tip_partials=tv)
    return t


def written(ot):
    return [k for k in ot.plk if np.any(ot.plk[k] != 0)]


SHAPES = [(300, 96, 7, False), (301, 96, 7, False), (40, 8230, 3, False), (20, 131200, 5, False), (40, 8230, 3, True)]


@pytest.mark.parametrize("n_otu,P,seed,ambiguous", SHAPES)
def test_every_internal_buffer_is_the_oracles(n_otu, P, seed, ambiguous):
    ot, ref, tree, tv, wg = reference(n_otu, P, seed, ambiguous)
    t, t0 = device_tree(ot, tree, tv, wg, P), device_tree(ot, tree, tv, wg, P)
    try:
        t0.inst.set_virtual_buffers(0)
        lnl, lnl0 = t.Lk(None), t0.Lk(None)
        print(f"{n_otu} x {P}: lnL {lnl!r} all-stored {lnl0!r} oracle {ref!r}, virtual {t.inst.virtual_stats()}")
        assert lnl == lnl0
        assert abs(lnl - ref) / abs(ref) < 1e-12
        # the default run computes its tip x tip results inside the steps that read them; the companion stores every one
        assert t.inst.virtual_stats()[0] > 0 and t0.inst.virtual_stats() == (0, 0, 0, 0)
        keys = written(ot)
        assert len(keys) >= n_otu - 2
        for x in (t, t0):
            for k in keys:
                assert np.array_equal(x.partials(*k), ot.plk[k]), (k, x is t0)
                assert np.array_equal(x.scale_factors(*k), ot.scale[k]), (k, x is t0)
    finally:
        t.close(); t0.close()


def test_the_long_list_rescales_unevenly_inside_a_wave():
    """The inputs decide something: at the 300-taxon shape the oracle's scale exponents are non-zero, and differ between the 32
    patterns that share a two-lane wave -- a maximum exchanged with the wrong lane, or not at all, changes them.  And in the
    ambiguous alignment an all-ones result (exactly 1.0 in every entry of a column) does reach an internal buffer."""
    for n_otu in (300, 301):
        ot = reference(n_otu, 96, 7, False)[0]
        uneven = 0
        for k in written(ot):
            sc = np.asarray(ot.scale[k]).reshape(-1)[:96]
            for w in range(0, 96, 32):
                uneven += int(sc[w:w + 32].max() > 0 and sc[w:w + 32].min() != sc[w:w + 32].max())
        assert uneven > 0, n_otu
    ot = reference(40, 8230, 3, True)[0]
    ones = sum(int(np.any(np.all(np.asarray(ot.plk[k]).reshape(8230, -1) == 1.0, axis=1))) for k in written(ot))
    assert ones >= 2, ones  # the cherry and the node above it
