"""ML_Dist restated -- TEST INFRASTRUCTURE, this repository's own code, independent of the product's device code.

For every pair of taxa (src/lk.c:1783-1906): the counts F with numpy, the starting value as K80_dist / JC69_Dist form it
(src/utilities.c:2407-2587) with math.pow / math.log, then Opt_Dist_F / Dist_F_Brent (src/optimiz.c:1848-1972) transcribed line by
line on -Lk_Dist (src/lk.c:2416-2473): matrices through orc.pmat_edge (one category of rate 1: PMat_Empirical's doubles), math.log,
the sum in the reference's order with plain products and additions.  What it leaves to the reference binary is its compiler's
contraction (measured: tests/test_mldist_restatement.py).
"""
import math

import numpy as np

import orc

DIST_MAX = 2.0
SMALL = 2.2250738585072014e-308
NT_STATE = {ord(c): i for i, c in enumerate("ACGT")}
AA_STATE = {ord(c): i for i, c in enumerate("ARNDCQEGHILKMFPSTWYV")}
AA_STATE[ord("B")] = AA_STATE[ord("N")]   # the single states N / Q on this ABI
AA_STATE[ord("Z")] = AA_STATE[ord("Q")]


def states_of(chars, ns):
    """[n][P] characters -> the one state of each cell, or -1 where the character allows several"""
    lut = np.full(256, -1, np.int64)
    for c, s in (NT_STATE if ns == 4 else AA_STATE).items():
        lut[c] = s
    return lut[np.asarray(chars, dtype=np.uint8)]


def pair_list(n):
    return [(j, k) for j in range(n - 1) for k in range(j + 1, n)]


def raw_counts(states, wght, ns):
    """[pair][ns][ns] sums of the weights (above SMALL) of the patterns where both taxa have one state"""
    st = np.asarray(states)
    n = st.shape[0]
    w = np.where(np.asarray(wght, dtype=np.float64) > SMALL, np.asarray(wght, dtype=np.float64), 0.0)
    out = np.zeros((n * (n - 1) // 2, ns, ns))
    for x, (j, k) in enumerate(pair_list(n)):
        ok = (st[j] >= 0) & (st[k] >= 0)
        np.add.at(out[x], (st[j][ok], st[k][ok]), w[ok])
    return out


def start_value(G, ns):
    """K80_dist(data, 1e6) (4 states) / JC69_Dist of one pair from its raw counts, BEFORE ML_Dist's 0.1 rule"""
    ln = float(G.sum())
    if ns == 4:
        ts = float(G[0, 2] + G[2, 0] + G[1, 3] + G[3, 1])
        tv = float(G.sum() - np.trace(G)) - ts
        P, Q = (ts / ln, tv / ln) if ln > 0.0 else (.5, .5)
        if (1 - 2 * P - Q <= .0) or (1 - 2 * Q <= .0):
            return -1.0
        g = 1.E+6
        d = (g / 2) * (math.pow(1 - 2 * P - Q, -1. / g) + 0.5 * math.pow(1 - 2 * Q, -1. / g) - 1.5)
    else:
        mis = float(G.sum() - np.trace(G))
        P = mis / ln if ln > 0.0 else 1.
        x = 1. - (ns) / (ns - 1.) * P
        if x < .0:
            return -1.0
        d = math.inf if x == 0.0 else -(ns - 1.) / (ns) * math.log(x)
    return min(d, DIST_MAX)


class Model:
    def __init__(self, pi, e_val, r_e_vect, l_e_vect, l_min, l_max):
        self.pi = [float(x) for x in np.asarray(pi).reshape(-1)]
        self.ns = len(self.pi)
        self.R, self.U, self.V = orc.f64(e_val), orc.f64(r_e_vect), orc.f64(l_e_vect)
        self.l_min, self.l_max = float(l_min), float(l_max)
        self.one = np.ones(1)

    def lk_dist(self, F, dist):
        ns = self.ns
        ln = min(max(dist, self.l_min), self.l_max)
        Pm = orc.pmat_edge(ln, ns, 1, self.one, 1.0, self.l_min, self.l_max, self.U, self.V, self.R)[0].tolist()
        lnL = .0
        for i in range(ns - 1):
            pi = self.pi[i]
            for j in range(i + 1, ns):
                lnL += (F[i][j] + F[j][i]) * math.log(pi * Pm[i][j])
        for i in range(ns):
            lnL += F[i][i] * math.log(self.pi[i] * Pm[i][i])
        return lnL


def sign(a, b):
    return abs(a) if b > 0.0 else -abs(a)


def dist_f_brent(ax, bx, cx, tol, n_iter_max, F, mod, min_diff_lk):
    """src/optimiz.c:1848-1953; returns (param, Lk_Dist at param, the iteration that returned)"""
    BRENT_CGOLD, BRENT_ZEPS = 0.3819660, 1.e-10
    e = 0.0
    d = 0.0
    a = ax if ax < cx else cx
    b = ax if ax > cx else cx
    x = w = v = bx
    old_lnL = -1.e20
    fw = fv = fx = -mod.lk_dist(F, abs(bx))
    curr_lnL = init_lnL = -fw
    for it in range(1, 1001):
        xm = 0.5 * (a + b)
        tol1 = tol * abs(x) + BRENT_ZEPS
        tol2 = 2.0 * tol1
        if ((abs(curr_lnL - old_lnL) < min_diff_lk) and (curr_lnL > init_lnL - min_diff_lk)) or (it > n_iter_max - 1):
            return x, mod.lk_dist(F, x), it
        if abs(e) > tol1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            etemp = e
            e = d
            if abs(p) >= abs(0.5 * q * etemp) or p <= q * (a - x) or p >= q * (b - x):
                e = a - x if x >= xm else b - x
                d = BRENT_CGOLD * e
            else:
                d = p / q
                u = x + d
                if u - a < tol2 or b - u < tol2:
                    d = sign(tol1, xm - x)
        else:
            e = a - x if x >= xm else b - x
            d = BRENT_CGOLD * e
        u = x + d if abs(d) >= tol1 else x + sign(tol1, d)
        old_lnL = curr_lnL
        fu = -mod.lk_dist(F, abs(u))
        curr_lnL = -fu
        if fu < fx:
            if u >= x:
                a = x
            else:
                b = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu < fw or abs(w - x) < SMALL:
                v = w; w = u; fv = fw; fw = fu
            elif fu < fv or abs(v - x) < SMALL or abs(v - w) < SMALL:
                v = u; fv = fu
    raise RuntimeError("Too many iterations in Dist_F_Brent")


def optimise_pair(F, init, mod, min_diff_lk):
    """One pair from its normalised counts F [ns][ns] and the closed form's value: (d, Lk_Dist at d before the cap, iterations)"""
    if init > DIST_MAX - SMALL or init < .0:
        init = 0.1
    Fl = np.asarray(F).tolist()
    s = 0.0
    for row in Fl:
        for x in row:
            s += x
    if s < .001:
        return init, 0.0, 0
    assert 1. - .001 < s < 1. + .001, s
    bx = mod.l_min if init < mod.l_min else init
    d, lnl, it = dist_f_brent(mod.l_min, bx, mod.l_max, 1.E-10, 1000, Fl, mod, min_diff_lk)
    return d, lnl, it


def ml_dist(chars, wght, mod, min_diff_lk, start=None, counts=None):
    """The whole of ML_Dist.  start: the [n][n] matrix of K80_dist / JC69_Dist (None: recomputed from the counts); counts: raw
    [pair][ns][ns] sums (None: numpy's, from chars).  Returns a dict: dist [n][n], start [n][n], F [pair][ns][ns], lnl [pair],
    iterations [pair]."""
    ns = mod.ns
    st = states_of(chars, ns)
    n = st.shape[0]
    G = raw_counts(st, wght, ns) if counts is None else np.asarray(counts)
    pairs = pair_list(n)
    D, S0 = np.zeros((n, n)), np.zeros((n, n))
    F = np.zeros_like(G)
    lnl, its = np.zeros(len(pairs)), np.zeros(len(pairs), np.int32)
    for x, (j, k) in enumerate(pairs):
        ln = float(G[x].sum())
        F[x] = G[x] / ln if ln > 0.0 else G[x]
        s0 = start_value(G[x], ns) if start is None else float(start[j][k])
        S0[j, k] = S0[k, j] = s0
        d, lnl[x], its[x] = optimise_pair(F[x], s0, mod, min_diff_lk)
        D[j, k] = D[k, j] = min(d, DIST_MAX)
    return {"dist": D, "start": S0, "F": F, "lnl": lnl, "iterations": its}


def model_of(fx):
    """The Model of a tests/golden/mldist_<case>.npz fixture"""
    return Model(fx["pi"], fx["e_val"], fx["r_e_vect"], fx["l_e_vect"], fx["l_min"][0], fx["l_max"][0])
