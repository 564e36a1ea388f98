"""The site loop of Ancestral_Sequences_One_Node (src/ancestral.c:609-901) restated in numpy over an orc.OracleTree -- TEST
INFRASTRUCTURE, the yardstick of phyhip_calculate_node_state_posteriors.

    x_k(c,i) = sum_j side_k[p][c][j] * Pij_k[c][i][j]      side_k: the partial vector of b_k on v_k's side; a tip: its 0/1 vector
    ss       = the scale exponents of the non-tip sides at p, added
    q[i]     = sum_c x_0 x_1 x_2 pi[i] gamma_r_proba[c]
    +I:        q[i] = q[i] (1 - pinvar) + Invariant_Lk(ss, p) pinvar pi[i];  where that overflowed: Invariant_Lk(0, p) pinvar pi[i]
    post[i]  = exp(log(q[i]) - LOG2 ss - c_lnL_sorted[p])

The tree must be in the state ot.lk(None, both_sides=True) leaves (every partial vector current).  tests/
test_ancestral_restatement.py holds this to the reference's own printed probabilities (tests/golden/ancestral_*.txt.gz).
"""
import gzip
import os

import numpy as np

LOG2 = 0.69314718055994528623  # src/utilities.h:267
SMALL = 2.2250738585072014e-308
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def internal_nodes(ot):
    return list(range(ot.n, 2 * ot.n - 2))


def node_sides(ot, d):
    """[(neighbour, edge, side of the edge the neighbour sits on)] of internal node d, in the tree's neighbour order"""
    return [(v, be, 1 if d == ot.el[be] else 0) for (v, be) in ot.adj[d]]


def node_posteriors(ot, nodes=None, site_lnl=None, zero_unweighted=True):
    """(post [node][pattern][state], numerical warning).  site_lnl: c_lnL_sorted (default: the oracle tree's own, as its last
    lk() left it).  zero_unweighted: rows of patterns whose weight is not above SMALL are zero (what the device writes; the
    reference reads stale vectors there)."""
    m = ot.m
    S, Cc, P = m.ns, m.ncatg, ot.P
    nodes = internal_nodes(ot) if nodes is None else list(nodes)
    lnl = np.asarray(ot.c_lnL_sorted if site_lnl is None else site_lnl, dtype=np.float64)
    pi = np.asarray(m.pi, dtype=np.float64)
    cw = np.asarray(m.gamma_r_proba, dtype=np.float64)
    weighted = ot.wght > SMALL
    out = np.zeros((len(nodes), P, S))
    warn = 0
    with np.errstate(all="ignore"):
        for k, d in enumerate(nodes):
            sides = node_sides(ot, d)
            assert len(sides) == 3, d
            prod = None
            ss = np.zeros(P, np.int64)
            for (v, be, side) in sides:
                if v < ot.n:
                    x = np.broadcast_to(np.asarray(ot.tip_vec[v]).reshape(P, 1, S), (P, Cc, S))
                else:
                    x = ot.plk[(be, side)].reshape(P, Cc, S)
                    ss += ot.scale[(be, side)]
                xk = np.einsum("pcj,cij->pci", x, ot.pm[be])
                prod = xk if prod is None else prod * xk
            q = (prod * pi[None, None, :] * cw[None, :, None]).sum(axis=1)
            if m.invar_model:
                iv = np.asarray(ot.invar, dtype=np.int64)
                inv0 = np.where(iv >= 0, pi[np.clip(iv, 0, S - 1)], 0.0)          # Invariant_Lk(0, p)
                inv = np.ldexp(inv0, ss.astype(np.int64)) if ot.apply_scaling else inv0   # Invariant_Lk(ss, p): pi * 2^ss piecewise, exact
                over = np.isinf(inv)
                q = np.where(over[:, None], (inv0 * m.pinvar)[:, None] * pi[None, :],
                             q * (1.0 - m.pinvar) + (inv * m.pinvar)[:, None] * pi[None, :])
                if np.any(over & weighted):
                    warn = 1
            out[k] = np.exp(np.log(q) - LOG2 * ss[:, None] - lnl[:, None])
            if zero_unweighted:
                out[k][~weighted] = 0.0
    return out, warn


def load_reference_file(name, n_otu, n_sites, ns):
    """tests/golden/ancestral_<name>.txt.gz, the reference's *_phyml_ancestral_seq.txt of a --no_colalias run: (printed
    probabilities [n_otu - 2][n_sites][ns] with row k = node n_otu + k, the set of (node, site) rows present)."""
    out = np.full((n_otu - 2, n_sites, ns), np.nan)
    seen = set()
    for line in gzip.open(os.path.join(GOLDEN, "ancestral_" + name + ".txt.gz"), "rt"):
        f = line.split()
        if len(f) < 2 + ns or not (f[0].isdigit() and f[1].isdigit()):
            continue
        site, node = int(f[0]) - 1, int(f[1])
        out[node - n_otu, site] = [float(x) for x in f[2:2 + ns]]
        seen.add((node, site))
    return out, seen
