"""tests/mldist_ref.py (ML_Dist restated: numpy counts, the oracle's matrices, math.log / math.pow, Dist_F_Brent line by line) against
the REAL reference's own ML_Dist matrices (tests/golden/mldist_<case>.npz, written by tests/golden/make_mldist.py), every pair of
all four fixtures.  CPU-only.

Bounds (set by what separates the two, not by what the code gives): the restatement follows the reference's trajectory and differs
by the reference binary's contraction only -- measured when the fixtures were made: nucleic 1.0e-10 worst relative (559 of 1431
pairs bit-equal), proteic 2.5e-11, designed_nt 1.6e-13, designed_aa 1.7e-13 -- while a pair that took another branch of the optimiser lands orders of
magnitude away: 1e-9 relative.  Starting values recomputed from the counts: the reference's bits on 4 states, 1e-14 relative on 20
states (contraction in 1 - c P; measured 1.2e-15).
"""
import os

import numpy as np
import pytest

import mldist_ref as mr
from conftest import GOLDEN

CASES = ["nucleic", "proteic", "designed_nt", "designed_aa"]
_cache = {}


def restated(name):
    """(fixture, restatement run with the reference's starting matrix, starting values recomputed from the counts) -- computed once"""
    if name not in _cache:
        fx = dict(np.load(os.path.join(GOLDEN, "mldist_" + name + ".npz")))
        mod = mr.model_of(fx)
        r = mr.ml_dist(fx["chars"], fx["wght"], mod, float(fx["min_diff_lk_local"][0]), start=fx["start"])
        G = mr.raw_counts(mr.states_of(fx["chars"], mod.ns), fx["wght"], mod.ns)
        n = fx["chars"].shape[0]
        s0 = np.zeros((n, n))
        for x, (j, k) in enumerate(mr.pair_list(n)):
            s0[j, k] = s0[k, j] = mr.start_value(G[x], mod.ns)
        _cache[name] = (fx, r, s0)
    return _cache[name]


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_distances_follow_the_reference(name):
    fx, r, _ = restated(name)
    n = fx["chars"].shape[0]
    iu = np.triu_indices(n, 1)
    worst = rel(r["dist"][iu], fx["dist"][iu]).max()
    print(f"{name}: {len(iu[0])} pairs, worst relative difference {worst:.3g}, bit-equal {(r['dist'][iu] == fx['dist'][iu]).sum()}, "
          f"iterations {r['iterations'].min()}..{r['iterations'].max()}")
    assert worst < 1e-9, worst
    assert np.array_equal(r["dist"], r["dist"].T) and not r["dist"].diagonal().any()


@pytest.mark.parametrize("name", CASES)
def test_starting_values_from_the_counts(name):
    fx, _, s0 = restated(name)
    if fx["pi"].size == 4:
        assert np.array_equal(s0, fx["start"])
    else:
        d = rel(s0, fx["start"])
        print(f"{name}: worst relative difference of the starting values {d.max():.3g}, {(s0 != fx['start']).sum() // 2} pairs differ")
        assert d.max() < 1e-14


@pytest.mark.parametrize("name", ["designed_nt", "designed_aa"])
def test_the_designed_branches(name):
    fx, r, _ = restated(name)
    D, l_min = r["dist"], float(fx["l_min"][0])
    pairs = mr.pair_list(D.shape[0])
    at = lambda key: tuple(int(v) for v in fx["pair_" + key])
    j, k = at("identical")
    assert D[j, k] == l_min and fx["dist"][j, k] == l_min
    j, k = at("disjoint")
    assert D[j, k] == 0.1 and fx["start"][j, k] == -1.0 and r["iterations"][pairs.index((j, k))] == 0
    j, k = at("saturated")
    assert D[j, k] == 2.0 and fx["start"][j, k] == -1.0 and r["iterations"][pairs.index((j, k))] > 0
    j, k = at("over")
    assert fx["start"][j, k] == 2.0 and rel(D[j, k], fx["dist"][j, k]) < 1e-9
