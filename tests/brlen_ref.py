"""Br_Len_Spline (src/optimiz.c:2244-2470) restated in Python over any callable dlk(l) -> (l_clamped, lnL, dlnL): the search that
phyhip_optimise_edge_length runs in its kernel (phyml_amd/csrc/phyhip_brlen.hip) and that the host layer's Br_Len_Opt drives probe by
probe where that call is not built.  What it does, not what it seems to mean:
  * init_lnL is the caller's c_lnL (the matrix route's Lk(b)): what fv becomes when the first derivative is already negative, and
    what best_lnL starts from -- the first probe's own lnL is never compared with it;
  * best_l starts as the UNCLAMPED start, and the upper walk restarts from it;
  * the resets *l = 0.5 / *l = 0.001 sit behind a dLk that has already clamped;
  * u - v < DBL_MIN is true whenever u < v: the do-while normally runs once;
  * new_l keeps its initial -1. when neither root is accepted and u / v lies within [0.9, 1.1].
Python floats are IEEE doubles and every product, quotient and sqrt below is rounded where it stands, as the C is compiled.

Besides the result the search returns every decision it took with its margin -- how far the compared quantity was from flipping the
branch -- so that a caller can tell which records a last-bit difference in the sums could send down another path:
  "sign"  |dlnL| at the sign tests of the two walks and of the spline step      (units of dlnL)
  "best"  |lnL - best_lnL| at the best-so-far tests                             (units of lnL)
  "tol"   ||lnL - old_lnL| - tol| at the convergence test                       (units of lnL)
  "root"  the distance of the accepted root from u, v and from the 1e-5 bands  (units of l; compare with root_spread)
"""
import math
import sys
from collections import namedtuple

DBL_MIN = sys.float_info.min
BRENT_IT_MAX = 1000
SPLINE, LOWER, UPPER, NO_ROOT, BRACKET, TOO_LONG, NAN, CAP = range(8)

Result = namedtuple("Result", "l lnL dlnL evaluations status n_tot best_from decisions spline probes roots")


def ieee_div(x, y):
    """x / y as C's double division gives it: x / 0 = +-inf, 0 / 0 = nan (Python raises ZeroDivisionError there)"""
    try:
        return x / y
    except ZeroDivisionError:
        return float("nan") if x == 0.0 or x != x else math.copysign(float("inf"), x) * math.copysign(1.0, y)


def trip_cap(frm, l_max):
    """the trips a walk in factors of 1.2 can take between frm and l_max (the host-computed bound of the device call)"""
    span = math.log(l_max / frm) / math.log(1.2)
    if not (span > 0.0) or math.isinf(span):
        return 2
    return min(8192, int(math.ceil(span) + 2.0))


def spline_roots(u, v, fu, fv, dfu, dfv):
    """:2344-2356: (root1, root2) in units of l; nan where the reference's arithmetic gives one"""
    a_ = dfu * (v - u) - (fv - fu)
    b_ = -dfv * (v - u) + (fv - fu)
    A_ = 3. * a_ - 3. * b_
    B_ = -4. * a_ + 2. * b_
    C_ = fv - fu + a_
    disc = B_ * B_ - 4. * A_ * C_
    D_ = math.sqrt(disc) if disc >= 0.0 else float("nan")
    r1 = ieee_div(-B_ - D_, 2. * A_)
    r2 = ieee_div(-B_ + D_, 2. * A_)
    return r1 * (v - u) + u, r2 * (v - u) + u


def pick_root(u, v, root1, root2):
    """:2358-2376: (which, new_l or None) -- which: 1 / 2 the accepted root, 0 none but u / v within [0.9, 1.1], -1 the assert.
    u / v is the C division of :2372: u / 0 is +-inf (the assert), 0 / 0 is nan (neither comparison holds: no assert)"""
    ok1 = root1 > u and root1 < v
    ok2 = root2 > u and root2 < v
    if abs(root1 - u) < 1.E-5: ok1 = True
    if abs(root2 - u) < 1.E-5: ok2 = True
    if abs(root1 - v) < 1.E-5: ok1 = True
    if abs(root2 - v) < 1.E-5: ok2 = True
    if ok1 and ok2:
        return (1, root1) if root1 < root2 else (2, root2)
    if ok1:
        return 1, root1
    if ok2:
        return 2, root2
    q = ieee_div(u, v)
    if q > 1.1 or q < 0.9:
        return -1, None
    return 0, None


def root_margin(u, v, root1, root2):
    """how far the acceptance tests of both roots are from flipping, in units of l (nan roots: inf, they flip nothing)"""
    m = float("inf")
    for r in (root1, root2):
        if r != r:
            continue
        for edge in (u, v):
            d = abs(r - edge)
            m = min(m, d, abs(d - 1.E-5))
    if root1 == root1 and root2 == root2:
        m = min(m, abs(root1 - root2))
    return m


def root_spread(sp, b_lnl, b_dlnl):
    """the accepted root's largest move when fu, fv are moved by +-b_lnl and dfu, dfv by +-b_dlnl (sp: Result.spline)"""
    u, v, fu, fv, dfu, dfv, which, root = sp
    worst = 0.0
    for s in range(16):
        sg = [(1.0 if (s >> i) & 1 else -1.0) for i in range(4)]
        r = spline_roots(u, v, fu + sg[0] * b_lnl, fv + sg[1] * b_lnl, dfu + sg[2] * b_dlnl, dfv + sg[3] * b_dlnl)[which - 1]
        worst = max(worst, abs(r - root)) if r == r else float("inf")
    return worst


def br_len_spline(dlk, l0, init_lnL, l_min, l_max, n_iter_max=BRENT_IT_MAX, tol=1.E-3, cap=None):
    """Returns Result: l = best_l, lnL = best_lnL, dlnL = c_dlnL as the search leaves it, the dLk evaluations, the status word of
    phyhip_optimise_edge_length, n_tot (the growth of tree->n_tot_bl_opt), best_from ("start": best_l is the start itself,
    "geometric": a length of one of the two walks, "spline": the spline's root), the decisions [(kind, margin)], the spline step
    (u, v, fu, fv, dfu, dfv, which root, root) or None, the probes [(l, lnL, dlnL)], and per turn of the spline loop
    (u, v, root1, root2, which).  cap: the trips either walk may take (None: trip_cap(l_min, l_max), the device call's bound)."""
    dec, probes, roots = [], [], []
    state = dict(n=0, n_tot=0)

    def ev(l):
        lc, lnl, dl = dlk(l)
        state["n"] += 1
        probes.append((lc, lnl, dl))
        return lc, lnl, dl

    def out(l, lnl, dl, status, best_from, spline=None):
        return Result(l, lnl, dl, state["n"], status, state["n_tot"], best_from, dec, spline, probes, roots)

    if l0 != l0:
        return out(l0, init_lnL, 0.0, NAN, "start")
    mult = 1.2
    init_l = best_l = l0
    best_lnL = old_lnL = init_lnL
    best_from = "start"
    cap_lower = cap_upper = trip_cap(l_min, l_max) if cap is None else cap
    new_l = -1.

    l, c_lnL, c_dlnL = ev(l0)
    init_dl = c_dlnL
    if l > l_max: l = 0.5
    if l < l_min: l = 0.001

    trips = 0
    while True:
        dec.append(("sign", abs(c_dlnL)))
        if not c_dlnL < 0.0:
            break
        l = l / mult
        state["n_tot"] += 1
        if l < l_min:
            return out(best_l, best_lnL, c_dlnL, LOWER, best_from)
        if trips >= cap_lower:
            return out(best_l, best_lnL, c_dlnL, CAP, best_from)
        trips += 1
        l, c_lnL, c_dlnL = ev(l)
        dec.append(("best", abs(c_lnL - best_lnL)))
        if c_lnL > best_lnL:
            best_lnL, best_l, best_from = c_lnL, l, "geometric"
    u, fu, dfu = l, c_lnL, c_dlnL

    l, c_dlnL, c_lnL = init_l, init_dl, init_lnL
    trips = 0
    while True:
        dec.append(("sign", abs(c_dlnL)))
        if not c_dlnL > 0.0:
            break
        l = l * mult
        state["n_tot"] += 1
        if l > l_max:
            return out(best_l, best_lnL, c_dlnL, UPPER, best_from)
        if trips >= cap_upper:
            return out(best_l, best_lnL, c_dlnL, CAP, best_from)
        trips += 1
        l, c_lnL, c_dlnL = ev(l)
        dec.append(("best", abs(c_lnL - best_lnL)))
        if c_lnL > best_lnL:
            best_lnL, best_l, best_from = c_lnL, l, "geometric"
    v, fv, dfv = l, c_lnL, c_dlnL

    it = 0
    spline = None
    while True:
        root1, root2 = spline_roots(u, v, fu, fv, dfu, dfv)
        which, r = pick_root(u, v, root1, root2)
        roots.append((u, v, root1, root2, which))
        dec.append(("root", root_margin(u, v, root1, root2)))
        if which < 0:
            return out(best_l, best_lnL, c_dlnL, NO_ROOT, best_from, spline)
        if which > 0:
            new_l = r
            if spline is None:
                spline = (u, v, fu, fv, dfu, dfv, which, r)
        l = new_l
        state["n_tot"] += 1
        old_lnL = c_lnL
        if l != l:
            return out(best_l, best_lnL, c_dlnL, NAN, best_from, spline)
        l, c_lnL, c_dlnL = ev(l)
        dec.append(("best", abs(c_lnL - best_lnL)))
        if c_lnL > best_lnL:
            best_lnL, best_l, best_from = c_lnL, l, "spline"
        dec.append(("sign", abs(c_dlnL)))
        if c_dlnL > 0.0:
            u, fu, dfu = new_l, c_lnL, c_dlnL
        else:
            v, fv, dfv = new_l, c_lnL, c_dlnL
        converged = u - v < DBL_MIN
        if not converged:
            dec.append(("tol", abs(abs(c_lnL - old_lnL) - tol)))
        if abs(c_lnL - old_lnL) < tol:
            converged = True
        it += 1
        if it == n_iter_max + 20:
            converged = True
        if converged:
            break
        if not (u < v) or not (dfu > 0.0) or not (dfv < 0.0):
            return out(best_l, best_lnL, c_dlnL, BRACKET, best_from, spline)
    return out(best_l, best_lnL, c_dlnL, TOO_LONG if it == n_iter_max else SPLINE, best_from, spline)
