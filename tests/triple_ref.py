"""Triple_Dist (src/utilities.c:7120-7146) restated over the CPU oracle (orc.OracleTree) and brlen_ref.br_len_spline: the matrices of
a->b[1] and a->b[2], then per edge Update_Partial_Lk(tree, a->b[i], a) and Br_Len_Opt (src/optimiz.c:607-663: Lk(b) with
update_eigen_lr, Br_Len_Spline on the edge's products, *l = best_l, the matrix refresh, the lk_end check), then the partials of b[1]
and b[0] once more.  It changes the oracle tree as the reference changes its tree; restore() puts the three lengths and matrices back
(the caller re-runs lk(None, both_sides=True) where it needs the node's partials as they were)."""
from collections import namedtuple

import brlen_ref

LK_END = 8  # status: lk_end < lk_begin - tol, where the reference stops the program (src/optimiz.c:656)

Search = namedtuple("Search", "edge l_in lk_begin result status")
Triple = namedtuple("Triple", "edges searches lengths lnL n_tot evaluations")


def edges_of(ot, a):
    """a->b[0..2] in the tree's own neighbour order"""
    e = [be for (_, be) in ot.adj[a]]
    assert len(e) == 3, a
    return e


def br_len_opt(ot, e, iter_max=brlen_ref.BRENT_IT_MAX, tol=1.E-3, l_in=None):
    """Br_Len_Opt(&b->l, b, tree) on edge e (from l_in where given): Search with brlen_ref's Result; status is the Result's, or LK_END"""
    if l_in is not None:
        ot.len[e] = l_in
    l0 = float(ot.len[e])
    lkb = ot.lk(e)
    ot.update_eigen_lr(e)
    r = brlen_ref.br_len_spline(ot.dlk, l0, lkb, ot.m.l_min, ot.m.l_max, iter_max, tol)
    status = r.status
    if status < 3:
        ot.len[e] = r.l
        ot.update_pmat(e)
        if r.lnL < lkb - tol:
            status = LK_END
    return Search(e, l0, lkb, r, status)


def triple_dist(ot, a, iter_max=brlen_ref.BRENT_IT_MAX, tol=1.E-3, after_search=None):
    """Triple_Dist(a, tree) at internal node a.  Stops behind a search whose status is 3..8, as the reference stops the program.
    after_search(i, Search) runs behind search i while the oracle still holds that edge's products and exponents."""
    e = edges_of(ot, a)
    ot.update_pmat(e[1])
    ot.update_pmat(e[2])
    searches = []
    for i in range(3):
        ot.update_partial(e[i], a)
        searches.append(br_len_opt(ot, e[i], iter_max, tol))
        if after_search is not None:
            after_search(i, searches[-1])
        if searches[-1].status >= 3:
            break
    else:
        ot.update_partial(e[1], a)
        ot.update_partial(e[0], a)
    return Triple(e, searches, [float(ot.len[x]) for x in e], searches[-1].result.lnL, sum(s.result.n_tot for s in searches),
                  sum(s.result.evaluations for s in searches))


def restore(ot, edges, lengths):
    for e, l in zip(edges, lengths):
        ot.len[e] = l
        ot.update_pmat(e)
