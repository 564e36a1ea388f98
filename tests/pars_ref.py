"""A numpy restatement of the reference's parsimony code (src/pars.c) over operation lists, both modes -- the checker of the device
kernels (tests/test_gpu_parsimony.py), itself held to the reference's own dumps (tests/test_parsimony_restatement.py).

Buffers are numbered as the host layer numbers the partials buffers (Make_Tree_For_Lk): tips 0..n-1, then one per internal edge side
in edge order, left before right.  Fitch (src/pars.c:380-391, :432-433): a buffer is (ui, pars); step matrix (:357-376, :411-428):
p_pars [P][ns], every minimum starting from MAX_PARS, plain int arithmetic.  Tips: ui = the allowed-state mask, pars = 0; p_pars = 0
where allowed, MAX_PARS elsewhere (Init_Ui_Tips / Init_Partial_Pars_Tips)."""
import numpy as np

MAX_PARS = 1000000000

_NT = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "M": 3, "R": 5, "W": 9, "S": 6, "Y": 10, "K": 12, "B": 14, "D": 13, "H": 11, "V": 7,
       "N": 15, "X": 15, "?": 15, "O": 15, "-": 15}
_AA_ORDER = "ARNDCQEGHILKMFPSTWYV"
_AA = {c: 1 << i for i, c in enumerate(_AA_ORDER)}
_AA.update({"B": 1 << 2, "Z": 1 << 5, "X": (1 << 20) - 1, "?": (1 << 20) - 1, "-": (1 << 20) - 1})


def char_masks(seq, ns):
    """[n][P] characters (uint8) -> [n][P] allowed-state masks (src/lk.c:26-199)"""
    table = np.zeros(256, np.int64)
    for c, m in (_NT if ns == 4 else _AA).items():
        table[ord(c)] = m
    out = table[np.asarray(seq, dtype=np.uint8)]
    assert (out > 0).all()
    return out


def masks_to_partials(masks, ns):
    """[P] masks -> [P][ns] 0/1 doubles (a row of phyhip_set_tip_partials)"""
    return ((np.asarray(masks)[:, None] >> np.arange(ns)[None, :]) & 1).astype(np.float64)


def nt_step_mat():
    """transition 1, transversion 2, states in ACGT order"""
    m = np.full((4, 4), 2, np.int64)
    m[0, 2] = m[2, 0] = m[1, 3] = m[3, 1] = 1
    np.fill_diagonal(m, 0)
    return m


class Planes:
    """buffer index -> its values; tips from the masks, inner buffers as operations write them"""

    def __init__(self, masks, ns, step=None):
        self.masks, self.ns, self.n = np.asarray(masks, dtype=np.int64), ns, len(masks)
        self.step = None if step is None else np.asarray(step, dtype=np.int64).reshape(ns, ns)
        self.P = self.masks.shape[1]
        self.buf = {}

    @property
    def general(self):
        return self.step is not None

    def get(self, b):
        if b < self.n:
            m = self.masks[b]
            if self.general:
                return np.where(((m[:, None] >> np.arange(self.ns)[None, :]) & 1) == 1, 0, MAX_PARS).astype(np.int64)
            return m.copy(), np.zeros(self.P, np.int64)
        if b not in self.buf:  # a plane nothing has written yet holds zeros
            return np.zeros((self.P, self.ns), np.int64) if self.general else (np.zeros(self.P, np.int64), np.zeros(self.P, np.int64))
        return self.buf[b]

    def _side_min(self, v):
        # min(MAX_PARS, min_j(v[p][j] + step[i][j])) -> [P][ns]
        return np.minimum(MAX_PARS, (v[:, None, :] + self.step[None, :, :]).min(axis=2))

    def run(self, ops):
        for d, c1, c2 in ops:
            assert d >= self.n and d != c1 and d != c2
            if self.general:
                self.buf[d] = self._side_min(self.get(c1)) + self._side_min(self.get(c2))
            else:
                (u1, p1), (u2, p2) = self.get(c1), self.get(c2)
                ui, pars = u1 & u2, p1 + p2
                miss = ui == 0
                self.buf[d] = (np.where(miss, u1 | u2, ui), pars + miss)
        return self

    def site_pars(self, b1, b2):
        if self.general:
            return (self._side_min(self.get(b1)) + self._side_min(self.get(b2))).min(axis=1).clip(max=MAX_PARS)
        (u1, p1), (u2, p2) = self.get(b1), self.get(b2)
        return p1 + p2 + ((u1 & u2) == 0)


def weighted_sum(site, wght):
    """exact: python integers"""
    return sum(int(s) * int(w) for s, w in zip(site, wght))


def truncating_sum(site, wght):
    """the reference's own loop for any weights: c_pars (an int) += site_pars * wght (a double), truncated at every pattern"""
    c = 0
    for s, w in zip(site, wght):
        c = int(float(c) + float(int(s)) * float(w))
    return c


class TreeIndex:
    """the buffer numbering and the traversals of a dumped topology (edge ends + each node's v[] / b[] order)"""

    def __init__(self, n, edge_left, edge_rght, node_v, node_b):
        self.n, self.E = int(n), len(edge_left)
        self.left, self.rght = [int(x) for x in edge_left], [int(x) for x in edge_rght]
        self.v, self.b = np.asarray(node_v, dtype=np.int64), np.asarray(node_b, dtype=np.int64)
        nxt = self.n
        self.left_idx, self.rght_idx = [], []
        for e in range(self.E):
            assert self.left[e] >= self.n or self.n <= 2
            self.left_idx.append(nxt); nxt += 1
            if self.rght[e] < self.n:
                self.rght_idx.append(self.rght[e])
            else:
                self.rght_idx.append(nxt); nxt += 1
        self.nbuf = nxt

    def side(self, e, d):
        """buffer of edge e on node d's side"""
        return self.left_idx[e] if d == self.left[e] else self.rght_idx[e]

    def child(self, d, e):
        """buffer of the subtree seen from d across edge e"""
        return self.rght_idx[e] if d == self.left[e] else self.left_idx[e]

    def op(self, e, d):
        """Update_Partial_Pars(tree, edge e, node d): None for a tip"""
        if d < self.n:
            return None
        kids = [self.child(d, int(self.b[d][i])) for i in range(3) if int(self.b[d][i]) != e]
        assert len(kids) == 2
        return (self.side(e, d), kids[0], kids[1])

    def post_order(self, a, d, out):
        if d < self.n:
            return
        dr = -1
        for i in range(3):
            if int(self.v[d][i]) != a:
                self.post_order(d, int(self.v[d][i]), out)
            else:
                dr = i
        out.append(self.op(int(self.b[d][dr]), d))

    def pre_order(self, a, d, out):
        if d < self.n:
            return
        for i in range(3):
            if int(self.v[d][i]) != a:
                out.append(self.op(int(self.b[d][i]), d))
                self.pre_order(d, int(self.v[d][i]), out)

    def both_sides(self):
        """the operations of Pars(NULL) with both_sides == YES, in the reference's order"""
        out = []
        self.post_order(0, int(self.v[0][0]), out)
        self.pre_order(0, int(self.v[0][0]), out)
        return [o for o in out if o is not None]

    def post_only(self):
        out = []
        self.post_order(0, int(self.v[0][0]), out)
        return [o for o in out if o is not None]


def tree_of_fixture(d):
    return TreeIndex(int(d["n_otu"][0]), d["edge_left"], d["edge_rght"], d["node_v"], d["node_b"])


def random_tree(n, seed):
    """a random unrooted binary topology as (edge_left, edge_rght): tips 0..n-1 on the right of their edges"""
    rng = np.random.RandomState(seed)
    nxt = n
    edges = [(nxt, 0), (nxt, 1), (nxt, 2)]
    nxt += 1
    for t in range(3, n):
        a, b = edges.pop(rng.randint(len(edges)))
        edges += [(nxt, a) if a < n else (a, nxt), (nxt, b) if b < n else (b, nxt), (nxt, t)]
        nxt += 1
    edges = [(a, b) if b < n or a >= n else (b, a) for a, b in edges]
    return np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32)


def neighbours(n, edge_left, edge_rght):
    """v[] / b[] in edge order (Make_Tree_From_Edges without neighbour arrays)"""
    v = -np.ones((2 * n - 2, 3), np.int64); b = -np.ones((2 * n - 2, 3), np.int64)
    fill = [0] * (2 * n - 2)
    for e, (l, r) in enumerate(zip(edge_left, edge_rght)):
        for x, y in ((int(l), int(r)), (int(r), int(l))):
            v[x][fill[x]] = y; b[x][fill[x]] = e; fill[x] += 1
    return v, b
