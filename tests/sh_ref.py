"""An independent restatement (numpy, integers and IEEE doubles only) of the resampling behind SH-like branch supports as
phyhip_calculate_sh_support defines it (include/phyhip.h): the alias table of Sample_n_i_With_Proba_pi (src/stats.c:4493-4560),
Philox4x32-10, the draws, the sums (math.fsum beside them as the exact value), the two six-way orderings of src/alrt.c:1184-1216 /
1254-1287 and the counts.  tests/test_sh_restatement.py holds it to the real reference's recorded data; the GPU tests hold the
library to it.  No library code is used here."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
EPS = 2.0 ** -52


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (arrays of equal shape or scalars) under key (k0, k1): four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def alias_table(w, init_len):
    """(prob, alias) of Sample_n_i_With_Proba_pi(w / init_len, len(w), .), operation for operation"""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    pi = w / float(init_len)
    s = 0.0
    for x in pi:
        assert x >= 0
        s += float(x)
    assert s != 0.0
    p = [float(x) * n / s for x in pi]
    small, large = [], []
    for i in range(n - 1, -1, -1):
        (small if p[i] < 1 else large).append(i)
    prob, alias = np.zeros(n), np.zeros(n, np.int32)
    while small and large:
        a, g = small.pop(), large.pop()
        prob[a] = p[a]
        alias[a] = g
        p[g] = p[g] + p[a] - 1
        (small if p[g] < 1 else large).append(g)
    for i in large + small:
        prob[i] = 1.0
    return prob, alias


def sample_with_uniforms(prob, alias, u):
    """The reference's draw loop (src/stats.c:4566-4572) fed its own uniforms u = rand() / RAND_MAX, two per draw"""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    i = (len(prob) * u[:, 0]).astype(np.int64)
    return np.where(u[:, 1] < prob[i], i, alias[i]).astype(np.int32)


def draws(prob, alias, sites, replicates, seed, first=0):
    """[replicates][sites] drawn patterns of replicates first .. first + replicates - 1"""
    P = len(prob)
    pairs = (sites + 1) // 2
    j = np.arange(pairs, dtype=np.uint64)[None, :]
    r = np.arange(first, first + replicates, dtype=np.uint64)[:, None]
    w = philox4x32_10(j, 0, r, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((replicates, 2 * pairs), np.int32)
    for h in (0, 1):
        col = ((w[2 * h].astype(np.uint64) * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
        keep = w[2 * h + 1].astype(np.float64) * 2.0 ** -32 < prob[col]
        out[:, h::2] = np.where(keep, col, alias[col])
    return out[:, :sites]


def delta6(c0, c1, c2):
    """(delta, branch 0..5) by the six-way ordering of src/alrt.c:1184-1216, line by line"""
    c0, c1, c2 = (np.asarray(x, dtype=np.float64) for x in (c0, c1, c2))
    A = (c0 >= c1) & (c0 >= c2)
    B = ~A & (c1 >= c0) & (c1 >= c2)
    Cc = ~A & ~B
    br = np.where(A, np.where(c1 >= c2, 0, 1), np.where(B, np.where(c0 >= c2, 2, 3), np.where(c1 >= c0, 4, 5)))
    val = np.choose(br, [c0 - c1, c0 - c2, c1 - c0, c1 - c2, c2 - c1, c2 - c0])
    assert (A | B | Cc).all()
    return val, br


def totals(lks, w):
    """c_k in the reference's order, their exact values and the rounding bound P 2^-52 sum |terms|"""
    lks = np.asarray(lks, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    terms = lks * w[None, :]
    c = np.zeros(3)
    for p in range(lks.shape[1]):
        c = c + terms[:, p]
    exact = np.array([math.fsum(terms[k]) for k in range(3)])
    bound = lks.shape[1] * EPS * np.abs(terms).sum(axis=1)
    return c, exact, bound


def support(lks, w, sites, replicates, seed, table=None, idx=None, exact_rows=None):
    """Everything phyhip_calculate_sh_support returns, and what the tests need beside it.  exact_rows: the replicates whose sums are
    also formed exactly (math.fsum)."""
    lks = np.asarray(lks, dtype=np.float64)
    prob, alias = table if table is not None else alias_table(w, sites)
    if idx is None:
        idx = draws(prob, alias, sites, replicates, seed)
    c, c_exact, c_bound = totals(lks, w)
    sums, absum = np.zeros((replicates, 3)), np.zeros((replicates, 3))
    lt, at = np.ascontiguousarray(lks.T), np.ascontiguousarray(np.abs(lks).T)
    for s in range(sites):  # the reference's order: site by site
        sums += lt[idx[:, s]]
        absum += at[idx[:, s]]
    bound = sites * EPS * absum
    rell_flags = (sums[:, 0] >= sums[:, 1]) & (sums[:, 0] >= sums[:, 2])
    delta, br = delta6(*c)
    lk = sums - c[None, :]
    dl, brl = delta6(lk[:, 0], lk[:, 1], lk[:, 2])
    accepted = delta > (dl + 0.1)
    # decided: the margin exceeds 8 x the rounding bound of what enters it (each centred sum: its sum's bound + its total's)
    b = bound.max(axis=1) + c_bound.max()
    decided = np.abs(delta - dl - 0.1) > 8 * b
    bs = bound.max(axis=1)
    d1, d2 = sums[:, 0] - sums[:, 1], sums[:, 0] - sums[:, 2]
    rell_decided = ((np.abs(d1) > 8 * bs) & (np.abs(d2) > 8 * bs)) | (-d1 > 8 * bs) | (-d2 > 8 * bs)
    out = dict(prob=prob, alias=alias, idx=idx, totals=c, totals_exact=c_exact, totals_bound=c_bound, sums=sums, sums_bound=bound,
               delta=float(delta), delta_branch=int(br), delta_local=dl, local_branch=brl, accepted=accepted, rell_flags=rell_flags,
               decided=decided, rell_decided=rell_decided, sh=accepted.sum() / replicates, rell=rell_flags.sum() / replicates)
    if exact_rows is not None:
        rows = np.asarray(exact_rows)
        out["exact_rows"] = rows
        out["sums_exact"] = np.array([[math.fsum(lks[k, idx[r]].tolist()) for k in range(3)] for r in rows])
    return out


def mc_bound(a, b, replicates):
    """Five standard deviations of the difference of two independent estimates of one probability from `replicates` draws each, + 2/R"""
    p = 0.5 * (a + b)
    return 5.0 * math.sqrt(2.0 * p * (1.0 - p) / replicates) + 2.0 / replicates


def designed_triple(P, order, seed=3):
    """Three vectors [3][P] whose totals under unit weights are ordered as `order` (a permutation of 0, 1, 2: largest first) with clear
    gaps, and whose centred replicate sums fluctuate alike, so that delta_local takes every ordering across replicates: a common
    base, independent noise per vector, and a constant shift per vector (it moves c_k and every replicate's lk_k by the same amount
    when sites == sum of the weights)."""
    j = np.arange(P, dtype=np.uint64)
    u = lambda stream: philox4x32_10(j, stream, 0, 0, seed, 77)[0].astype(np.float64) * 2.0 ** -32
    base = -2.0 - 6.0 * u(1)
    noise = np.stack([u(10 + k) - 0.5 for k in range(3)])
    noise -= noise.mean(axis=1, keepdims=True)
    shift = np.zeros(3)
    shift[order[0]], shift[order[1]], shift[order[2]] = 0.02, 0.012, 0.0
    return base[None, :] + noise + shift[:, None]


# ---- what the CPU and the GPU tests share -----------------------------------------------------------------------------------------
SEED = 0x5EED0A17C0FFEE  # the seed of every test that compares flags (the CPU test holds the undecided share at this seed)
REPLICATES = 10000
_cache = {}


def fixture(name):
    """tests/golden/sh_support_<name>.npz"""
    import os
    if ("fx", name) not in _cache:
        here = os.path.dirname(os.path.abspath(__file__))
        _cache[("fx", name)] = dict(np.load(os.path.join(here, "golden", "sh_support_" + name + ".npz")))
    return _cache[("fx", name)]


def fixture_draws(name):
    """(prob, alias), the drawn patterns [REPLICATES][init_len] of a fixture's own weights at SEED: computed once, shared, left unchanged"""
    if ("idx", name) not in _cache:
        fx = fixture(name)
        sites = int(fx["init_len"][0])
        table = alias_table(fx["wght"], sites)
        idx = draws(table[0], table[1], sites, REPLICATES, SEED)
        idx.setflags(write=False)
        _cache[("idx", name)] = (table, idx)
    return _cache[("idx", name)]


def fixture_support(name, e, exact_rows=None):
    """The restatement of recorded edge e (position in the file) of a fixture at SEED"""
    key = ("sup", name, e, None if exact_rows is None else tuple(exact_rows))
    if key not in _cache:
        fx = fixture(name)
        table, idx = fixture_draws(name)
        _cache[key] = support(fx["lks"][e], fx["wght"], int(fx["init_len"][0]), REPLICATES, SEED, table=table, idx=idx, exact_rows=exact_rows)
    return _cache[key]


def picked_edges(name):
    """Positions of three recorded edges: the lowest support, the one nearest 0.5, the highest below 1"""
    sh = fixture(name)["sh"]
    below = np.where(sh < 1.0)[0]
    return [int(np.argmin(sh)), int(np.argmin(np.abs(sh - 0.5))), int(below[np.argmax(sh[below])])]


# the smallest shapes at which the kernels can still go wrong: one pattern, one below / at / above a wave of patterns, the fixture's;
# one and two sites (no whole pair / one pair), an odd count above a wave of pairs, the fixture's even count; 1, 3 and 10 000 replicates
SHAPES = [(1, 1, 1, "ones"), (1, 886, 3, "ones"), (63, 2, 3, "zeros"), (63, 127, 10000, "heavy"), (64, 127, 3, "ones"),
          (64, 886, 10000, "zeros"), (65, 1, 10000, "heavy"), (65, 2, 1, "fixture"), (65, 886, 3, "zeros"), (65, 127, 10000, "fixture"),
          (382, 127, 10000, "fixture"), (382, 1, 3, "heavy"), (382, 2, 10000, "ones"), (382, 886, 3, "zeros")]


def weights_of(kind, P):
    """The four weight vectors of tests/golden/sh_helper.c, cut to P patterns"""
    i = np.arange(P, dtype=np.uint64)
    if kind == "fixture":
        return fixture("nucleic")["wght"][:P].copy()
    if kind == "ones":
        return np.ones(P)
    if kind == "zeros":
        w = (((i * np.uint64(2654435761)) & MASK) >> np.uint64(13)) % np.uint64(4)
        w = w.astype(np.float64)
        if not w.any():
            w[0] = 2.0
        return w
    assert kind == "heavy"
    w = np.ones(P)
    w[P // 3] = 5.0 * P
    return w


def shape_case(P, sites, kind):
    """(vectors [3][P], weights [P]) of a shape: a recorded edge at the fixture's 382 patterns, a designed triple below -- and at
    one or two sites, where the recorded vectors (many patterns carry the same value in all three) would tie exactly in more than
    0.1 % of the replicates; exact ties have a test of their own (three identical vectors)"""
    w = weights_of(kind, P)
    lks = fixture("nucleic")["lks"][1] if P == 382 and sites > 2 else designed_triple(P, (1, 2, 0), seed=P)
    return np.ascontiguousarray(lks), w


def shape_support(P, sites, R, kind):
    key = ("shape", P, sites, R, kind)
    if key not in _cache:
        lks, w = shape_case(P, sites, kind)
        rows = np.arange(R) if R <= 3 else np.arange(0, R, 97)
        _cache[key] = (lks, w, support(lks, w, sites, R, SEED, exact_rows=rows))
    return _cache[key]
