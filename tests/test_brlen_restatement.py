"""tests/brlen_ref.py -- Br_Len_Spline restated in Python -- against the REAL reference's Br_Len_Opt, CPU-only.  The fixtures
tests/golden/brlen_<case>.npz (tests/golden/make_brlen.py) hold what the reference did on every edge of the tree of the committed
.phyg from six start lengths; the restatement is driven by OracleTree.update_eigen_lr / dlk on that tree.

At EVERY record it reproduces the growth of tree->n_tot_bl_opt, the evaluation count and the status: exact.  l_out is equal to the
reference's bits wherever the path's best_l is the start itself or a length of one of the two walks in factors of 1.2 (exact IEEE
operations on both sides).  The oracle's sums are the reference's to within their last one to three ulps, not to the bits (lk_begin
differs at 113 of the 1 685 records, by at most 3.3e-16 relative): measured largest relative differences, all three cases --
lk_begin 3.26e-16, c_lnL 1.08e-15, the spline's l_out 6.94e-12, and c_dlnL 1.765e-07: the spline's root inherits the last bits of
four sums, and c_dlnL is the derivative AT that root -- a sum of terms of both signs that nearly cancels at the optimum, so the
root's 7e-12 shows as 5.4e-09 absolute in it (profiles/brlen_opt.md).  Each quantity is held at eight times ITS OWN largest
difference.  Thin decisions were removed when the fixtures were made; no record is skipped here.

One correction since: brlen_ref.pick_root now divides as C does at src/optimiz.c:2372 (`u / 0` = +-inf, the assert; `0 / 0` = NaN,
no assert) where it answered NaN for every v == 0.  No record here has v == 0 -- every number above is unchanged -- which is why
these fixtures could not see it; tests/test_brlen_step_restatement.py, which holds phyhip_brlen_step.h to the restatement on
synthetic functions, did (the header was right), and keeps the case."""
import os

import numpy as np
import pytest

import brlen_ref
import orc
import phyg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("nucleic_gtr_g4", "nucleic_gtr_g4_inv", "proteic_lg_g4")
REL = {"lk_begin": 8 * 3.26e-16, "c_lnL": 8 * 1.08e-15, "l_out": 8 * 6.94e-12, "c_dlnL": 8 * 1.765e-07}


@pytest.fixture(scope="module", params=CASES)
def replayed(request):
    name = request.param
    f = np.load(os.path.join(ROOT, "tests", "golden", "brlen_" + name + ".npz"))
    d = phyg.load(os.path.join(ROOT, "tests", "golden", name + ".phyg"))
    ot = orc.tree_from_golden(d)
    ot.lk(None, both_sides=True)
    assert np.array_equal(f["edge_len"], d["edge_len"])
    res = []
    for i in range(len(f["edge"])):
        e, l_in = int(f["edge"][i]), float(f["l_in"][i])
        ot.len[e] = l_in
        lkb = ot.lk(e)
        ot.update_eigen_lr(e)
        res.append((lkb, brlen_ref.br_len_spline(ot.dlk, l_in, lkb, float(f["l_min"][0]), float(f["l_max"][0]), int(f["iter_max"][0]),
                                                 float(f["tol"][0]))))
        ot.len[e] = float(d["edge_len"][e])
        ot.update_pmat(e)
    return name, f, res


def test_every_start_of_every_edge_is_there(replayed):
    name, f, res = replayed
    n_edges = len(f["edge_len"])
    assert len(res) + len(f["dropped"]) == 6 * n_edges and len(f["dropped"]) * 10 <= 6 * n_edges
    assert set(int(s) for s in f["start"]) == set(range(6))
    ev = f["evaluations"]
    assert (ev <= 2).any() and ((ev > 2) & (ev <= 8)).any() and (ev >= 32).any()      # the short, the ordinary and the long walks
    assert (f["status"] == 1).any() and (f["status"] == 0).any()


def test_counts_and_statuses_are_the_references(replayed):
    name, f, res = replayed
    for i, (_, r) in enumerate(res):
        assert r.n_tot == int(f["n_tot"][i]), (name, i)
        assert r.evaluations == int(f["evaluations"][i]) and r.status == int(f["status"][i]), (name, i)
        assert r.status in (0, 1, 2) and r.evaluations == r.n_tot + (0 if r.status in (1, 2) else 1), (name, i)
        assert {"start": 0, "geometric": 1, "spline": 2}[r.best_from] == int(f["best_from"][i]), (name, i)


def test_a_start_below_l_min_and_a_negative_start_on_a_near_zero_edge(replayed):
    name, f, res = replayed
    seen = 0
    for i, (_, r) in enumerate(res):
        if int(f["start"][i]) in (3, 5) and int(f["status"][i]) == 1 and int(f["evaluations"][i]) == 1:
            assert r.l == float(f["l_in"][i]) == float(f["l_out"][i])       # one evaluation, l left as it was
            seen += 1
    assert seen > 0


def test_lengths_and_likelihoods(replayed):
    name, f, res = replayed
    worst = {k: 0.0 for k in REL}
    for i, (lkb, r) in enumerate(res):
        if r.best_from != "spline":
            assert r.l == float(f["l_out"][i]), (name, i, r.l.hex(), float(f["l_out"][i]).hex())
        for key, got in (("lk_begin", lkb), ("l_out", r.l), ("c_lnL", r.lnL), ("c_dlnL", r.dlnL)):
            want = float(f[key][i])
            rel = abs(got - want) / max(abs(want), 1e-300)
            worst[key] = max(worst[key], rel)
            assert rel <= REL[key], (name, i, key, got, want, rel)
    print(name, "largest relative differences", {k: "%.3e" % v for k, v in worst.items()})
