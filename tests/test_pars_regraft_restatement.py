"""The reference's recorded parsimony SPR candidates (tests/golden/regraft_pars_<case>.npz: Prune_Subtree, then Graft_Subtree,
Pars(NULL) with both sides, Pars(b_arrow) for every edge of the residual tree) equal what tests/pars_ref.py's join and score give on
the three operand vectors of each candidate, built over the pruned topology by tests/pars_regraft_ref.py -- c_pars at every
candidate of all four cases, site_pars where the fixture keeps it, both modes.  Integers, ==, no tolerance.  This pins the fixture
and the bookkeeping tests/test_gpu_pars_regraft.py reuses, without a GPU."""
import os

import numpy as np
import pytest

import pars_ref
import pars_regraft_ref as rr


def test_the_fixtures_are_all_there():
    for case in rr.CASES:
        base, rg = rr.load(case)
        n = int(base["n_otu"][0])
        assert os.path.getsize(os.path.join(rr.HERE, "golden", "regraft_pars_%s.npz" % case)) < 1000 * 1000
        K, T = rg["prune"].shape[0], rg["target_edge"].shape[0]
        assert rg["target_off"][0] == 0 and rg["target_off"][-1] == T and len(rg["target_off"]) == K + 1
        assert rg["c_pars_fitch"].shape == (T,) and rg["c_pars_general"].shape == (T,)
        if case.startswith("designed"):
            # every prune site in both directions: an internal edge twice, a tip edge once; site_pars kept
            internal = int(((base["edge_left"] >= n) & (base["edge_rght"] >= n)).sum())
            assert K == 2 * internal + n
            assert rg["site_fitch"].shape == (T, base["wght"].shape[0]) == rg["site_general"].shape
        else:
            assert K == 6 and "site_fitch" not in rg
            assert (rg["prune"][:, 2] < n).any(), "a tip as the subtree"
            assert (rg["target_ends"] < n).any(), "a tip at an end of a target edge"
        # every target of the residual tree: the whole tree's edges but the arrow, the subtree's own and the one pruning merges away
        for s in rr.sites(case):
            sub_tips = _tips_behind(base, s.link, s.dsub)
            assert len(s.rows) == (2 * n - 3) - 2 - (2 * sub_tips - 2), (case, s.edge, s.link)


def _tips_behind(base, a, d):
    n = int(base["n_otu"][0])
    if d < n:
        return 1
    return sum(_tips_behind(base, d, int(c)) for c in base["node_v"][d] if int(c) != a)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("case", rr.CASES)
def test_join_and_score_equal_the_reference(case, general):
    base, rg = rr.load(case)
    c_key, s_key = ("c_pars_general", "site_general") if general else ("c_pars_fitch", "site_fitch")
    for s in rr.sites(case):
        pl = rr.planes(base, general).run(s.ops)
        for r, cand in zip(s.rows, s.cands):
            _, site = rr.join_and_score(pl, s.spare, cand)
            assert pars_ref.weighted_sum(site, base["wght"]) == int(rg[c_key][r]), (case, s.edge, s.link, r)
            if s_key in rg:
                assert np.array_equal(site, rg[s_key][r]), (case, s.edge, s.link, r)


@pytest.mark.parametrize("case", ["designed_nt", "designed_aa"])
def test_regrafting_where_it_was_pruned_gives_the_whole_tree(case):
    """the candidate on the edge pruning merged is the tree of pars_<case>.npz itself: the reference's Pars(b) there"""
    base, rg = rr.load(case)
    for s in rr.sites(case):
        hits = 0
        for r in s.rows:
            e = int(rg["target_edge"][r])
            if s.link in (int(base["edge_left"][e]), int(base["edge_rght"][e])):
                hits += 1
                assert int(rg["c_pars_fitch"][r]) == int(base["cpars_fitch"][s.edge])
                assert int(rg["c_pars_general"][r]) == int(base["cpars_general"][s.edge])
                assert np.array_equal(rg["site_fitch"][r], base["site_fitch"][s.edge])
                assert np.array_equal(rg["site_general"][r], base["site_general"][s.edge])
        assert hits == 1
