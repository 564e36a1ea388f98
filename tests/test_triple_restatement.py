"""tests/triple_ref.py -- Triple_Dist restated over the CPU oracle and tests/brlen_ref.py -- against the REAL reference's Triple_Dist,
CPU-only.  The fixtures tests/golden/triple_<case>.npz (tests/golden/make_triple.py) hold what the reference did at every internal
node of the tree of the committed .phyg, from the committed lengths and with the node's three edges scaled by 0.05 and by 20.

At EVERY record the restatement reproduces the growth of tree->n_tot_bl_opt, and the evaluation counts, statuses and paths the
fixture carries for the three searches: exact.  The lengths and c_lnL follow tests/test_brlen_restatement.py's rules for one search:
a length is equal to the reference's bits wherever the path's best_l is the start itself or a length of one of the two walks in
factors of 1.2 -- here for as long as no earlier search of the record, whose result the later ones start from, has ended on a spline
root -- and every length and c_lnL lie within that file's relative bounds (eight times the largest difference measured there over
1 685 single searches: l_out 6.94e-12, c_lnL 1.08e-15).  Thin decisions were removed when the fixtures were made; no record is
skipped here."""
import os

import numpy as np
import pytest

import orc
import phyg
import triple_ref
from test_brlen_restatement import REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("nucleic_gtr_g4", "nucleic_gtr_g4_inv", "proteic_lg_g4")
BEST_FROM = {"start": 0, "geometric": 1, "spline": 2}


@pytest.fixture(scope="module", params=CASES)
def replayed(request):
    name = request.param
    f = np.load(os.path.join(ROOT, "tests", "golden", "triple_" + name + ".npz"))
    d = phyg.load(os.path.join(ROOT, "tests", "golden", name + ".phyg"))
    ot = orc.tree_from_golden(d)
    ot.lk(None, both_sides=True)
    assert np.array_equal(f["edge_len"], d["edge_len"])
    res = []
    for i in range(len(f["node"])):
        a, edges = int(f["node"][i]), [int(e) for e in f["edges"][i]]
        assert triple_ref.edges_of(ot, a) == edges
        l0 = [float(d["edge_len"][e]) for e in edges]
        for e, l in zip(edges, f["l_in"][i]):
            ot.len[e] = float(l)
        res.append(triple_ref.triple_dist(ot, a, int(f["iter_max"][0]), float(f["tol"][0])))
        triple_ref.restore(ot, edges, l0)
        for e in edges:
            ot.update_partial(e, a)
    return name, f, d, res


def test_every_scaling_of_every_internal_node_is_there(replayed):
    name, f, d, res = replayed
    n = len(d["node_v"]) // 2 + 1
    assert len(res) + len(f["dropped"]) == 3 * (n - 2) and len(f["dropped"]) * 10 <= 3 * (n - 2)
    assert set(float(s) for s in f["scale"]) == {1.0, 0.05, 20.0}
    for i in range(len(res)):
        e = [int(x) for x in f["edges"][i]]
        assert [float(x) for x in f["l_in"][i]] == [min(float(d["edge_len"][x]) * float(f["scale"][i]), 90.0) for x in e]
    ev = f["evaluations"]
    assert (ev <= 2).any() and ((ev > 2) & (ev <= 8)).any() and (ev >= 32).any()      # the short, the ordinary and the long walks
    assert (f["status"] == 1).any() and (f["status"] == 0).any()


def test_counts_and_statuses_are_the_references(replayed):
    name, f, d, res = replayed
    for i, t in enumerate(res):
        assert t.n_tot == int(f["n_tot"][i]), (name, i)
        assert len(t.searches) == 3
        for k, s in enumerate(t.searches):
            r = s.result
            assert (r.evaluations, s.status, BEST_FROM[r.best_from]) == (int(f["evaluations"][i][k]), int(f["status"][i][k]), int(f["best_from"][i][k])), (name, i, k)
            assert s.status in (0, 1, 2) and r.evaluations == r.n_tot + (0 if s.status in (1, 2) else 1), (name, i, k)
        assert t.n_tot == sum(ev - 1 + (1 if st in (1, 2) else 0) for ev, st in zip(f["evaluations"][i], f["status"][i]))   # Br_Len_Opt's rule


def test_lengths_and_likelihoods(replayed):
    name, f, d, res = replayed
    worst = {"l_out": 0.0, "c_lnL": 0.0}
    for i, t in enumerate(res):
        exact = True
        for k, s in enumerate(t.searches):
            exact = exact and s.result.best_from != "spline"
            got, want = t.lengths[k], float(f["l_out"][i][k])
            if exact:
                assert got == want, (name, i, k, got.hex(), want.hex())
            rel = abs(got - want) / max(abs(want), 1e-300)
            worst["l_out"] = max(worst["l_out"], rel)
            assert rel <= REL["l_out"], (name, i, k, got, want, rel)
        rel = abs(t.lnL - float(f["lnL"][i])) / abs(float(f["lnL"][i]))
        worst["c_lnL"] = max(worst["c_lnL"], rel)
        assert rel <= REL["c_lnL"], (name, i, t.lnL, float(f["lnL"][i]), rel)
    print(name, "largest relative differences", {k: "%.3e" % v for k, v in worst.items()})
