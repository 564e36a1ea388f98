"""tests/pars_ref.py -- the numpy restatement the device kernels are checked against -- equals every vector the REAL reference
dumped (tests/golden/pars_<case>.npz, written by tests/golden/make_pars.py): both sides of every edge after Pars(NULL) with both
sides, site_pars and c_pars of Pars(b) at EVERY edge, in both modes.  Integers, np.array_equal, no tolerance.  CPU-only."""
import glob
import os

import numpy as np
import pytest

import pars_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(HERE, "golden", "pars_*.npz")))


def load(case):
    return dict(np.load(os.path.join(HERE, "golden", "pars_%s.npz" % case)))


def test_the_fixtures_are_all_there():
    assert CASES == sorted(["nucleic_bionj", "nucleic_random1", "nucleic_random2", "proteic_bionj", "proteic_random1", "proteic_random2",
                            "designed_nt", "designed_aa"])
    for case in CASES:
        d = load(case)
        assert os.path.getsize(os.path.join(HERE, "golden", "pars_%s.npz" % case)) < 1000 * 1000
        assert ("ppars" in d) == (case.startswith("designed") or case.endswith("bionj")), case
        if case.startswith("designed"):
            assert int(d["n_otu"][0]) == 9 and d["seq"].shape[1] < 100
            w, seq = d["wght"], d["seq"]
            amb = set(b"X?-NO") if d["ns"][0] == 4 else set(b"X?-")
            assert any(len(set(seq[:, p])) == 1 and seq[0, p] not in amb for p in range(len(w))), "a constant column"
            assert any(set(seq[:, p]) <= amb for p in range(len(w))), "a fully ambiguous column"
            assert any(len(set(seq[:, p])) == 9 for p in range(len(w))), "an all-different column"
            assert w.max() >= 2


@pytest.mark.parametrize("case", CASES)
def test_fitch_equals_the_reference(case):
    d = load(case)
    ns, T = int(d["ns"][0]), pars_ref.tree_of_fixture(d)
    pl = pars_ref.Planes(pars_ref.char_masks(d["seq"], ns), ns).run(T.both_sides())
    for e in range(T.E):
        for s, b in ((0, T.left_idx[e]), (1, T.rght_idx[e])):
            ui, pars = pl.get(b)
            assert np.array_equal(ui, d["ui"][e][s]) and np.array_equal(pars, d["pars"][e][s]), (case, e, s)
        site = pl.site_pars(T.left_idx[e], T.rght_idx[e])
        assert np.array_equal(site, d["site_fitch"][e]), (case, e)
        assert pars_ref.weighted_sum(site, d["wght"]) == int(d["cpars_fitch"][e]) == pars_ref.truncating_sum(site, d["wght"])


@pytest.mark.parametrize("case", CASES)
def test_step_matrix_equals_the_reference(case):
    d = load(case)
    ns, T = int(d["ns"][0]), pars_ref.tree_of_fixture(d)
    if ns == 4:
        assert np.array_equal(d["step_mat"], pars_ref.nt_step_mat())   # the product's own rule is the reference's table
    pl = pars_ref.Planes(pars_ref.char_masks(d["seq"], ns), ns, d["step_mat"]).run(T.both_sides())
    for e in range(T.E):
        if "ppars" in d:
            for s, b in ((0, T.left_idx[e]), (1, T.rght_idx[e])):
                assert np.array_equal(pl.get(b), d["ppars"][e][s]), (case, e, s)
        site = pl.site_pars(T.left_idx[e], T.rght_idx[e])
        assert np.array_equal(site, d["site_general"][e]), (case, e)
        assert pars_ref.weighted_sum(site, d["wght"]) == int(d["cpars_general"][e])


def test_the_truncating_loop_restated():
    """c_pars is an int: every pattern's product loses its fraction as it is added (src/pars.c:47)"""
    site = np.array([3, 1, 2, 5]); w = np.array([0.5, 0.5, 1.25, 0.1])
    assert pars_ref.truncating_sum(site, w) == 3          # 1.5 -> 1, +0.5 -> 1, +2.5 -> 3, +0.5 -> 3; the exact sum is 5
    assert pars_ref.truncating_sum(site, np.array([2.0, 1.0, 3.0, 1.0])) == pars_ref.weighted_sum(site, [2, 1, 3, 1]) == 18
