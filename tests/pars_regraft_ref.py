"""The bookkeeping of the parsimony regraft scan's checks: the reference's recorded SPR candidates (tests/golden/regraft_pars_<case>.npz,
written by tests/golden/make_pars_regraft.py) as operation lists and candidate records over the PRUNED topology, in buffer numbers a
device instance can use as they are.  tests/test_pars_regraft_restatement.py holds this bookkeeping and tests/pars_ref.py's join and
score to the reference's numbers without a GPU; tests/test_gpu_pars_regraft.py runs the same lists on the device.

The recursion is this module's own, over the fixture's node_v: vec(a, d) is the vector of the subtree behind d seen from its
neighbour a -- a tip, or the join of vec(d, c) over d's two other neighbours.  Pruning the subtree behind `dsub` at its link node
leaves the link's two other neighbours v1 and v2 adjacent: seen from v1 the link node passes its one remaining child (v2) through,
and the other way round."""
import os

import numpy as np

import pars_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["designed_nt", "designed_aa", "nucleic_bionj", "proteic_bionj"]
_cache = {}


def load(case):
    """(pars_<case>.npz, regraft_pars_<case>.npz)"""
    if case not in _cache:
        _cache[case] = (dict(np.load(os.path.join(HERE, "golden", "pars_%s.npz" % case))),
                        dict(np.load(os.path.join(HERE, "golden", "regraft_pars_%s.npz" % case))))
    return _cache[case]


class Site:
    """one recorded prune site: ops (dest, child1, child2) that build every vector its candidates name, in dependency order;
    cands [(child1, child2, subtree)] in the fixture's order; rows: their rows in the fixture; nbuf: buffers an instance needs
    (one spare behind the last vector: `spare`)"""

    def __init__(self, base, rg, k):
        n = self.n = int(base["n_otu"][0])
        v = [[int(x) for x in row if int(x) >= 0] for row in base["node_v"]]
        edge, link, dsub = (int(x) for x in rg["prune"][k])
        ends = {int(base["edge_left"][edge]), int(base["edge_rght"][edge])}
        assert ends == {link, dsub} and link >= n
        v1, v2 = [x for x in v[link] if x != dsub]
        self.edge, self.link, self.dsub = edge, link, dsub

        def nb(x):   # neighbours in the pruned tree (the subtree's own nodes keep theirs)
            return [(v2 if x == v1 else v1) if (y == link and x in (v1, v2)) else y for y in v[x]]

        self.ops, memo, nxt = [], {}, [n]

        def vec(a, d):
            if d < n:
                return d
            if (a, d) not in memo:
                kids = [c for c in nb(d) if c != a]
                assert len(kids) == 2, (a, d, kids)
                c1, c2 = vec(d, kids[0]), vec(d, kids[1])
                memo[(a, d)] = nxt[0]
                self.ops.append((nxt[0], c1, c2))
                nxt[0] += 1
            return memo[(a, d)]

        self.sub = vec(link, dsub)
        self.rows = list(range(int(rg["target_off"][k]), int(rg["target_off"][k + 1])))
        self.cands = []
        left, rght = base["edge_left"], base["edge_rght"]
        for r in self.rows:
            x, y = (int(t) for t in rg["target_ends"][r])
            e = int(rg["target_edge"][r])
            assert y in nb(x) and x in nb(y) and link not in (x, y)
            # the recorded edge number names this edge: its ends in the whole tree, the link node replaced by what pruning joined
            whole = {int(left[e]), int(rght[e])}
            assert whole == {x, y} or (link in whole and {x, y} == {v1, v2}), (e, whole, x, y)
            self.cands.append((vec(y, x), vec(x, y), self.sub))
        self.spare = nxt[0]
        self.nbuf = nxt[0] + 1


def sites(case):
    base, rg = load(case)
    return [Site(base, rg, k) for k in range(rg["prune"].shape[0])]


def planes(base, general):
    ns = int(base["ns"][0])
    return pars_ref.Planes(pars_ref.char_masks(base["seq"], ns), ns, base["step_mat"] if general else None)


def join_and_score(pl, spare, cand):
    """(J, site[]) of one candidate on a Planes that holds its three operands"""
    c1, c2, sub = cand
    pl.run([(spare, c1, c2)])
    return pl.get(spare), pl.site_pars(spare, sub)
