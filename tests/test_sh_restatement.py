"""tests/sh_ref.py -- the restatement the GPU tests hold phyhip_calculate_sh_support to -- against what does not depend on this
project: the published Philox4x32-10 known-answer vectors, and the REAL reference's recorded data (tests/golden/sh_support_*.npz:
its alias sampler against its own rand() stream, its Statistics_To_SH / Statistics_to_RELL per internal edge).  CPU-only; no
library code runs here."""
import itertools

import numpy as np
import pytest

import sh_ref as sr

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = sr.philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]


def test_philox_is_elementwise():
    j = np.arange(5)
    a = sr.philox4x32_10(j, 0, 7, 0, 1, 2)
    for i in range(5):
        assert [int(x[i]) for x in a] == [int(x) for x in sr.philox4x32_10(i, 0, 7, 0, 1, 2)]


@pytest.mark.parametrize("name", ["nucleic", "proteic"])
@pytest.mark.parametrize("v", range(4))
def test_alias_table_returns_the_references_indices(name, v):
    """The restatement's table, fed the reference's own rand() values as r / RAND_MAX, returns the indices its sampler returned"""
    fx = sr.fixture(name)
    w = fx["alias_w"][v]
    assert (v != 1 or (w == 1).all()) and (v != 2 or (w == 0).sum() > len(w) // 8) and (v != 3 or w.max() > w.sum() / 2)
    prob, alias = sr.alias_table(w, int(fx["init_len"][0]))
    u = fx["alias_rand"][v].astype(np.float64) / float(fx["rand_max"][0])
    got = sr.sample_with_uniforms(prob, alias, u)
    assert np.array_equal(got, fx["alias_idx"][v])
    assert ((prob >= 0) & (prob <= 1)).all() and (alias >= 0).all() and (alias < len(w)).all()
    assert (prob[w == 0] == 0).all() and (w[alias[prob < 1]] > 0).all()   # a pattern of no weight is never drawn


@pytest.mark.parametrize("name", ["nucleic", "proteic"])
def test_the_draws_follow_the_weights(name):
    """The drawn patterns' frequencies against w / sum w: a chi-square over the patterns within five standard deviations"""
    fx = sr.fixture(name)
    _, idx = sr.fixture_draws(name)
    w = fx["wght"]
    n = idx.size
    cnt = np.bincount(idx.ravel(), minlength=len(w))
    e = n * w / w.sum()
    chi2 = ((cnt - e) ** 2 / e).sum()
    dof = len(w) - 1
    assert abs(chi2 - dof) < 5 * np.sqrt(2 * dof), (chi2, dof)


@pytest.mark.parametrize("name", ["nucleic", "proteic"])
def test_supports_against_the_reference(name):
    """For every recorded edge: SH and RELL with 10 000 replicates within 5 sqrt(2 p (1 - p) / R) + 2 / R of the reference's,
    p the mean of the two (two independent Monte-Carlo estimates of one probability)"""
    fx = sr.fixture(name)
    assert len(fx["edges"]) >= 12
    worst = 0.0
    for e in range(len(fx["edges"])):
        s = sr.fixture_support(name, e)
        for got, ref in ((s["sh"], fx["sh"][e]), (s["rell"], fx["rell"][e])):
            b = sr.mc_bound(got, ref, sr.REPLICATES)
            worst = max(worst, abs(got - ref) / b)
            assert abs(got - ref) <= b, (name, int(fx["edges"][e]), got, ref, b)
    print(f"{name}: worst |difference| / bound over {len(fx['edges'])} edges: {worst:.2f}")


@pytest.mark.parametrize("name", ["nucleic", "proteic"])
def test_undecided_replicates_stay_under_the_cap(name):
    """The edges and the seed the GPU test compares flags at: the replicates whose margin does not exceed 8 x the rounding bound
    (expected: none, the bound is ~1e-9) stay under 0.1 %; the sums lie within their bound of the exact sums"""
    rows = np.arange(0, sr.REPLICATES, 97)
    for e in sr.picked_edges(name):
        s = sr.fixture_support(name, e, exact_rows=rows)
        assert (~s["decided"]).sum() <= sr.REPLICATES // 1000 and (~s["rell_decided"]).sum() <= sr.REPLICATES // 1000
        assert (np.abs(s["sums"][rows] - s["sums_exact"]) <= s["sums_bound"][rows]).all()
        assert (np.abs(s["totals"] - s["totals_exact"]) <= s["totals_bound"]).all()
        print(name, e, "undecided", int((~s["decided"]).sum()), int((~s["rell_decided"]).sum()), "largest bound", s["sums_bound"].max())


def test_designed_triples_take_every_ordering():
    """Six triples, one per ordering of the totals; across the replicates delta_local takes all six"""
    P = 65
    seen = set()
    for order in itertools.permutations(range(3)):
        lks = sr.designed_triple(P, order)
        s = sr.support(lks, np.ones(P), P, 3000, sr.SEED)
        c = s["totals"]
        assert c[order[0]] > c[order[1]] > c[order[2]]
        seen.add(s["delta_branch"])
        assert set(np.unique(s["local_branch"])) == set(range(6)), order
        assert 0 < s["accepted"].sum() < 3000
        assert (~s["decided"]).sum() <= 3
    assert seen == set(range(6))


def test_identical_vectors_have_no_support():
    fx = sr.fixture("nucleic")
    l = fx["lks"][0][0]
    table, idx = sr.fixture_draws("nucleic")
    s = sr.support(np.stack([l, l, l]), fx["wght"], int(fx["init_len"][0]), 500, sr.SEED, table=table, idx=idx[:500])
    assert s["sh"] == 0.0 and s["rell"] == 1.0 and s["delta"] == 0.0


def test_the_orderings_keep_their_ties():
    """>= at every comparison, as src/alrt.c:1184-1216 has it"""
    for c, want in (((1, 1, 1), (0, 0)), ((2, 2, 1), (0, 0)), ((2, 1, 2), (0, 1)), ((1, 2, 2), (0, 2 + 1)), ((1, 2, 1), (1, 2)),
                    ((1, 1, 2), (1, 4)), ((0, 1, 2), (1, 4)), ((1, 0, 2), (1, 5)), ((0, 2, 1), (1, 3))):
        d, br = sr.delta6(*[float(x) for x in c])
        assert (float(d), int(br)) == (float(want[0]), want[1]), (c, d, br)


@pytest.mark.parametrize("P,sites,R,kind", sr.SHAPES)
def test_the_small_shapes_stay_under_the_cap_too(P, sites, R, kind):
    """The shapes the GPU test runs: every weight vector is what it says, no replicate is undecided beyond 0.1 %"""
    lks, w, s = sr.shape_support(P, sites, R, kind)
    assert s["idx"].shape == (R, sites) and (w[s["idx"]] > 0).all()
    assert (~s["decided"]).sum() <= R // 1000 and (~s["rell_decided"]).sum() <= R // 1000
    assert (np.abs(s["sums"][s["exact_rows"]] - s["sums_exact"]) <= s["sums_bound"][s["exact_rows"]]).all()
