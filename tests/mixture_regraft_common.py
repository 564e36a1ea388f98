"""The reference of the mixture regraft scan's tests (tests/test_gpu_mixture_regraft.py, tests/test_mixture_regraft_restatement.py), CPU
only: per class the CPU oracle at buffer level -- orc_update_partial into a spare vector, then orc_edge_lnl, whose
unscaled_site_lk_cat / fact_sum_scale outputs are the class likelihood x_k and the exponent f_k -- and the site loop of MIXT_Lk over
the classes (phyml_amd.replay.mixture_combine; `combine` below restates it with the +I step of src/mixt.c:1086-1116 and the two
warnings, and is held to mixture_combine's bits wherever there is no +I)."""
import ctypes as C
import os

import numpy as np

import orc
from conftest import GOLDEN
from phyml_amd import phyg, replay

LEFT = 1          # PHYHIP_REGRAFT_SUBTREE_IS_LEFT
BAR = 1e-11       # tests/test_gpu_regraft.py's bar, for its reasons
TINY = np.finfo(np.float64).tiny   # SMALL = DBL_MIN


def fixture(name):
    """(dump, class models, (proba, r_w, e_w) per class, (r_sum, e_sum, sum_probas)) of tests/golden/mixture_<name>.phyg"""
    d = phyg.load(os.path.join(GOLDEN, "mixture_%s.phyg" % name))
    models, factors = replay.mixture_classes(d)
    return d, models, factors, (float(d["r_mat_weight_sum"][0]), float(d["e_frq_weight_sum"][0]), float(d["sum_probas"][0]))


class ClassChecker:
    """tests/test_gpu_regraft.py's Checker for one class tree, returning what the combination needs as well: buffers = {buffer
    index: (partials, exponents)}; an index below n_otu is the oracle tree's tip."""

    def __init__(self, ot, buffers):
        self.ot, self.buf = ot, buffers

    def side(self, idx):
        ot, s = self.ot, orc.Side()
        if idx < ot.n:
            s.p_lk = orc._p(ot.tip_vec[idx]); s.sum_scale = None; s.is_tip = 1
            s.is_ambigu = orc._p(ot.tip_amb[idx]); s.d_state = orc._p(ot.tip_ds[idx])
        else:
            p, sc = self.buf[idx]
            s.p_lk = orc._p(p); s.sum_scale = orc._p(sc); s.is_tip = 0; s.is_ambigu = None; s.d_state = None
        return s

    def pmat(self, l):
        m = self.ot.m
        return orc.pmat_edge(l, m.ns, m.ncatg, m.gamma_rr, m.br_len_mult, m.l_min, m.l_max, m.r_e_vect, m.l_e_vect, m.e_val)[0]

    def candidate(self, cand):
        """(x [P], f [P], computed vector [P][S], its exponents [P], the three matrices) of one record in this class"""
        c1, c2, sub, flags, l1, l2, l3 = cand
        ot, m, L = self.ot, self.ot.m, orc.lib()
        assert m.ncatg == 1
        pm = [np.ascontiguousarray(self.pmat(l)) for l in (l1, l2, l3)]
        vec = np.zeros((ot.P, m.ns)); sc = np.zeros(ot.P, np.int32)
        s1, s2 = self.side(c1), self.side(c2)
        L.orc_update_partial(C.c_int(ot.P), C.c_int(1), C.c_int(m.ns), orc._p(ot.wght), C.byref(s1), orc._p(pm[0]), C.byref(s2),
                             orc._p(pm[1]), orc._p(vec), orc._p(sc), C.c_int(ot.apply_scaling), C.c_int(ot.arith))
        comp = orc.Side()
        comp.p_lk = orc._p(vec); comp.sum_scale = orc._p(sc); comp.is_tip = 0; comp.is_ambigu = None; comp.d_state = None
        left, rght = (self.side(sub), comp) if flags & LEFT else (comp, self.side(sub))
        warn = C.c_int(0)
        a, b, x, f = np.zeros(ot.P), np.zeros(ot.P), np.zeros((ot.P, 1)), np.zeros(ot.P, np.int32)
        L.orc_edge_lnl(C.c_int(ot.P), C.c_int(1), C.c_int(m.ns), orc._p(ot.wght), C.byref(left), C.byref(rght), orc._p(pm[2]),
                       orc._p(m.pi), orc._p(m.gamma_r_proba), C.c_int(0), C.c_double(0.0), None, C.c_int(ot.apply_scaling), C.c_int(ot.arith),
                       orc._p(a), orc._p(b), orc._p(x), orc._p(f), C.byref(warn))
        return x[:, 0].copy(), f, vec, sc, pm


def combine(xs, fs, factors, sums, wght, invariant=None):
    """The site loop of MIXT_Lk (src/mixt.c:1027-1142) as phyml_amd.replay.mixture_combine restates it, plus -- invariant = (pinvar,
    invar [P], pi of the invariant class) -- the one step of src/mixt.c:1086-1116 between the class sum and the floor, and the two
    warnings at patterns with weight: an exponent above 1024, a site likelihood below SMALL.  Returns (lnL, warning)."""
    r_sum, e_sum, sum_probas = sums
    wght = np.asarray(wght, dtype=np.float64)
    has_w = wght > TINY
    site_lk = np.zeros(len(wght))
    warn = False
    for x, f, (proba, rw, ew) in zip(xs, fs, factors):
        f = np.asarray(f)
        warn = warn or bool(np.any((f > 1024) & has_w))
        s = np.where(f > 1024, 1023.0, np.minimum(f.astype(np.float64), 1024.0))
        with np.errstate(over="ignore"):
            u = np.asarray(x, dtype=np.float64) / np.power(2.0, s)
        site_lk = site_lk + u * proba * rw / r_sum * ew / e_sum / sum_probas
    if invariant is not None:
        pinvar, invar, pi_inv = invariant
        inv = np.where(np.asarray(invar) >= 0, np.asarray(pi_inv)[np.maximum(np.asarray(invar), 0)], 0.0)
        site_lk = site_lk * (1. - pinvar) + inv * pinvar
    warn = warn or bool(np.any((site_lk < TINY) & has_w))
    logs = np.log(np.maximum(site_lk, TINY))
    lnl = 0.0
    for p in range(len(wght)):
        if has_w[p]:
            lnl += wght[p] * logs[p]
    return lnl, int(warn)


def mixture_candidate(checkers, factors, sums, cand, invariant=None):
    """(lnL, warning, per-class (x, f, vector, exponents, matrices)) of one record over the class list"""
    per = [c.candidate(cand) for c in checkers]
    wght = checkers[0].ot.wght
    lnl, warn = combine([r[0] for r in per], [r[1] for r in per], factors, sums, wght, invariant)
    if invariant is None:   # the restatement above IS mixture_combine there
        ref, _ = replay.mixture_combine([r[0] for r in per], [r[1] for r in per], factors, sums[0], sums[1], sums[2], np.where(wght > TINY, wght, 0.0))
        assert ref == lnl, (ref, lnl)
    return lnl, warn, per


def within_bar(got, ref):
    return abs(got - ref) <= BAR * abs(ref)


def class_oracles(models, n, edge_left, edge_rght, edge_len, wght, tip_vec, tip_ds, tip_amb, apply_scaling=1):
    """one oracle tree per class model on the same topology, lengths and alignment, rooted as MIXT_Lk roots them"""
    out = []
    for md in models:
        ot = orc.OracleTree(orc.Model(md), n, edge_left, edge_rght, edge_len, wght, tip_vec, tip_ds, tip_amb, apply_scaling=apply_scaling)
        ot.tip_root = 0   # src/mixt.c:889
        out.append(ot)
    return out


def in_place_candidate(ot, index_of):
    """Regrafting a subtree where it already is, at the edge MIXT_Lk evaluates: the two other neighbours of the left node of that
    edge with their edge lengths, the tip on its right side as the subtree on the edge's own length, flags 0.  index_of(edge, side):
    the buffer index of an internal side vector."""
    e = ot.root_edge()
    d, tip = int(ot.el[e]), int(ot.er[e])
    assert d >= ot.n and tip < ot.n
    (_, ch) = ot.op_for(e, d)
    idx = []
    for (be, side) in ch:
        node = int(ot.el[be] if side == 0 else ot.er[be])
        idx.append(node if node < ot.n else index_of(be, side))
    return (idx[0], idx[1], tip, 0, float(ot.len[ch[0][0]]), float(ot.len[ch[1][0]]), float(ot.len[e]))
