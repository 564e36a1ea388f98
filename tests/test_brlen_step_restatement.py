"""phyml_amd/csrc/phyhip_brlen_step.h -- the one statement of Br_Len_Spline's control flow, compiled into the two search kernels and
into the host layer -- compiled by gcc for the host and held to its restatement tests/brlen_ref.py, CPU-only, on paths that real
likelihoods never take.  A small C program (written into tmp_path, as tests/test_exp_port.py does) runs brlen_begin / brlen_step on
recorded responses, clamping st.l to [l_min, l_max] in front of each step as the kernels do; the responses are the probes of
brlen_ref.br_len_spline over a seeded family of synthetic dlk callables: smooth unimodal, oscillating, derivatives inconsistent with
the values (exact zeros among them), NaN and +-inf regions, constant-sign tiny slopes.  Every probe length, best_l, best_lnL,
c_dlnL, the evaluation count and the status are equal to the bits (NaN equal to NaN), and the program needs exactly the responses
it is given.

What the family reaches is asserted on the restatement's results alone, before the C program runs: a property of the inputs.  One
property the search has by construction is asserted with it: the spline loop never takes a second turn.  u - v < DBL_MIN (:2405) is
true whenever u < v; where it is false (u >= v, or a NaN among them) the loop goes on only if |c_lnL - old_lnL| >= tol too, and then
assert(u < v) (:2423) fails -- status 4.  So the exit `u - v >= DBL_MIN` is followed by the tolerance test's convergence or by status
4, never by another iteration; both continuations are counted.

brlen_ref.pick_root divides as IEEE does since this module was written: `u / v if v != 0.0 else nan` took u > 0, v == 0 for "no
assert" where the reference's text, `else if(u/v > 1.1 || u/v < 0.9)` (src/optimiz.c:2372), divides in C: +inf > 1.1, the assert --
status 3.  The header was right and the restatement wrong; test_a_zero_start_with_a_nan_derivative keeps the case."""
import os
import random
import subprocess
import sys

import pytest

import brlen_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEARCHES = 24000
AT_LEAST = 50
INF, NAN = float("inf"), float("nan")

SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include "%s/phyml_amd/csrc/phyhip_brlen_step.h"
/* per search: "l0 init_lnL tol l_min l_max iter_max cap n" and n lines "lnL dlnL"; out: "n_probes probe... best_l best_lnL c_dlnL
   evals status used given" -- used == given + 1 where the program wanted one response more than it was given */
int main(int argc, char **argv)
{
  FILE *f = fopen(argv[1], "r");
  char w[5][64];
  int  it, cap, n;
  if (!f || argc < 2) return 2;
  while (fscanf(f, "%%63s %%63s %%63s %%63s %%63s %%d %%d %%d", w[0], w[1], w[2], w[3], w[4], &it, &cap, &n) == 8)
  {
    double *r = (double *)malloc(sizeof(double) * 2 * (n + 1)), *probe = (double *)malloc(sizeof(double) * (n + 1));
    const double l_min = strtod(w[3], NULL), l_max = strtod(w[4], NULL);
    BrlenState st;
    int k = 0;
    for (int i = 0; i < n; ++i)
    {
      char x[64], y[64];
      if (fscanf(f, "%%63s %%63s", x, y) != 2) return 3;
      r[2 * i] = strtod(x, NULL); r[2 * i + 1] = strtod(y, NULL);
    }
    brlen_begin(&st, strtod(w[0], NULL), strtod(w[1], NULL), strtod(w[2], NULL), l_min, l_max, it, cap);
    while (!st.done)
    {
      double l = st.l;
      if (l < l_min) l = l_min;
      else if (l > l_max) l = l_max;
      if (k >= n) { ++k; break; }
      probe[k] = l;
      st.l = l;
      brlen_step(&st, r[2 * k], r[2 * k + 1], 0);
      ++k;
    }
    printf("%%d", k > n ? n : k);
    for (int i = 0; i < (k > n ? n : k); ++i) printf(" %%a", probe[i]);
    printf(" %%a %%a %%a %%d %%d %%d %%d\n", st.best_l, st.best_lnL, st.c_dlnL, st.evals, st.status, k, n);
    free(r); free(probe);
  }
  fclose(f);
  return 0;
}
"""


# ---- the synthetic family: pure functions of the clamped length ---------------------------------------------------------------------
def _family(rng, l_min, l_max):
    """(kind, f): f(l) -> (lnL, dlnL) at the clamped length l"""
    import math
    kind = rng.choice(("unimodal", "unimodal", "oscillating", "oscillating", "inconsistent", "inconsistent", "inconsistent", "zeros",
                       "holes", "holes", "tiny", "flat"))
    m = math.exp(rng.uniform(math.log(max(l_min, 1e-6)), math.log(l_max)))      # where the optimum sits
    a = 10.0 ** rng.uniform(-2, 4)
    c = -10.0 ** rng.uniform(0, 5)
    if kind == "unimodal":          # a * (log l - l / m): the shape of one edge's likelihood, optimum at m
        def f(l):
            return c + a * (math.log(l) - l / m), a * (1.0 / l - 1.0 / m)
    elif kind == "oscillating":
        w, b = 10.0 ** rng.uniform(-1, 3), a * rng.uniform(0.1, 3.0)

        def f(l):
            x = w * l
            if x > 1e15:                # (sin of a huge argument is still a pure function of l; keep it cheap and finite)
                x = math.fmod(x, 6.0)
            return c - a * (l - m) ** 2 + b * math.sin(x), -2.0 * a * (l - m) + b * w * math.cos(x)
    elif kind == "inconsistent":    # the values of one function, the derivative of another: the cubic's roots land anywhere
        m2 = math.exp(rng.uniform(math.log(max(l_min, 1e-6)), math.log(l_max)))
        sgn = rng.choice((1.0, 1.0, -1.0))
        a2 = 10.0 ** rng.uniform(-3, 3)

        def f(l):
            return c - a * abs(l - m) ** rng_pow, sgn * a2 * (m2 - l)
        rng_pow = rng.choice((0.5, 1.0, 2.0, 3.0))
    elif kind == "zeros":           # a derivative quantised to a grid, exactly 0.0 around m; the value follows it or is constant
        q = m * rng.choice((0.05, 0.5, 2.0))
        flatv = rng.random() < 0.5

        def f(l):
            d = float(int((m - l) / q))
            return (c if flatv else c - a * (l - m) ** 2), a * d * q
    elif kind == "holes":           # a unimodal function with a region where the value or the derivative is nan / +inf / -inf
        lo = math.exp(rng.uniform(math.log(max(l_min, 1e-6)), math.log(l_max)))
        hi = lo * rng.choice((1.5, 10.0, 1e6))
        bad_v = rng.choice((None, NAN, INF, -INF))
        bad_d = rng.choice((NAN, INF, -INF)) if bad_v is None else rng.choice((None, NAN, INF, -INF))
        below = rng.random() < 0.3     # the region is everything below lo instead

        def f(l):
            v, d = c + a * (math.log(l) - l / m), a * (1.0 / l - 1.0 / m)
            if (l <= lo) if below else (lo <= l <= hi):
                return (v if bad_v is None else bad_v), (d if bad_d is None else bad_d)
            return v, d
    elif kind == "tiny":            # a slope of one sign everywhere, tiny: the walks run to a bound or to the cap
        d = rng.choice((1.0, -1.0)) * rng.choice((5e-324, 1e-300, 1e-30, 1e-12))

        def f(l):
            return c + d * l, d
    else:                           # flat: the same value everywhere, a derivative that changes sign at m
        def f(l):
            return c, (1.0 if l < m else -1.0) * a
    return kind, f


def _searches(n, seed):
    """[(arguments of br_len_spline, Result)]"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        l_min, l_max = rng.choice(((1e-8, 100.0), (1e-4, 10.0), (0.01, 2.0), (1e-8, 1e-3)))
        kind, f = _family(rng, l_min, l_max)

        def dlk(l, f=f, l_min=l_min, l_max=l_max):
            lc = l_min if l < l_min else l_max if l > l_max else l
            v, d = f(lc)
            return lc, v, d
        inside = l_min * (l_max / l_min) ** rng.random()
        l0 = rng.choice((l_min / 3.0, l_min, inside, inside, inside, inside, l_max, 2.0 * l_max, 0.0, -1.0, 1e308, INF))
        start_lnl = dlk(l0)[1]
        init = rng.choice((start_lnl, start_lnl, start_lnl + rng.uniform(-2.0, 2.0), -10.0 ** rng.uniform(0, 5)))
        it = rng.choice((1, 2, 3, 1000))
        tol = rng.choice((1e-3, 1e-12, 1e-300, 10.0))
        cap = brlen_ref.trip_cap(l_min, l_max) if rng.random() < 0.9 else rng.choice((0, 1, 3, 10))
        args = (l0, init, l_min, l_max, it, tol, cap)
        out.append((kind, args, brlen_ref.br_len_spline(dlk, *args)))
    return out


def _same(a, b):
    return (a != a and b != b) or (a == b and a.hex() == b.hex())


def _hx(x):
    return float(x).hex()


def _run_c(tmp_path, items):
    """items: [(l0, init_lnL, l_min, l_max, iter_max, tol, cap, [(lnL, dlnL)])] -> [(probes, best_l, best_lnL, c_dlnL, evals, status,
    used, given)] through the compiled header"""
    c = tmp_path / "step.c"
    c.write_text(SRC % ROOT)
    exe = str(tmp_path / "step")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, str(c), "-lm"])
    lines = []
    for (l0, init, l_min, l_max, it, tol, cap, resp) in items:
        lines.append("%s %s %s %s %s %d %d %d" % (_hx(l0), _hx(init), _hx(tol), _hx(l_min), _hx(l_max), it, cap, len(resp)))
        lines.extend("%s %s" % (_hx(v), _hx(d)) for v, d in resp)
    inp = tmp_path / "searches.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.returncode
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        n = int(w[0])
        out.append(([float.fromhex(x) for x in w[1:1 + n]],) + tuple(float.fromhex(x) for x in w[1 + n:4 + n]) + tuple(int(x) for x in w[4 + n:]))
    assert len(out) == len(items)
    return out


def _item(args, res, responses=None):
    l0, init, l_min, l_max, it, tol, cap = args
    return (l0, init, l_min, l_max, it, tol, cap, [(p[1], p[2]) for p in res.probes] if responses is None else responses)


def _assert_equal(what, res, got):
    probes, best_l, best_lnl, c_dlnl, evals, status, used, given = got
    assert used == given == len(res.probes), (what, "responses used / given / the restatement's", used, given, len(res.probes))
    assert len(probes) == len(res.probes) and all(_same(a, p[0]) for a, p in zip(probes, res.probes)), (what, probes, [p[0] for p in res.probes])
    assert (evals, status) == (res.evaluations, res.status), (what, evals, status, res.evaluations, res.status)
    assert _same(best_l, res.l) and _same(best_lnl, res.lnL) and _same(c_dlnl, res.dlnL), (what, (best_l, best_lnl, c_dlnl), (res.l, res.lnL, res.dlnL))


def _root_kinds(res):
    """of each turn of the spline loop: 'both' roots accepted, an accepted root 'band'-only (not inside (u, v)), 'kept' (none accepted,
    u / v within [0.9, 1.1], new_l stays)"""
    kinds = set()
    for (u, v, r1, r2, which) in res.roots:
        ok = [(r > u and r < v) or abs(r - u) < 1.E-5 or abs(r - v) < 1.E-5 for r in (r1, r2)]
        if ok[0] and ok[1]:
            kinds.add("both")
        if which > 0 and not ((r1, r2)[which - 1] > u and (r1, r2)[which - 1] < v):
            kinds.add("band")
        if which == 0:
            kinds.add("kept")
    return kinds


@pytest.fixture(scope="module")
def searches():
    return _searches(N_SEARCHES, seed=20)


def test_what_the_family_reaches(searches):
    """on the restatement's results alone: every status 0..5, the rare branches of the root choice, both continuations of the exit
    u - v >= DBL_MIN -- each at least 50 times -- and no second turn of the spline loop anywhere"""
    count = {}
    for kind, args, res in searches:
        keys = {("status", res.status)} | {("root", k) for k in _root_kinds(res)} | {("family", kind)}
        assert len(res.roots) <= 1, (args, "the spline loop took a second turn")
        if any(k == "tol" for k, _ in res.decisions):       # u - v < DBL_MIN was false behind the spline's probe
            assert res.status in (brlen_ref.SPLINE, brlen_ref.TOO_LONG, brlen_ref.BRACKET), (args, res.status)
            keys.add(("u - v >= DBL_MIN", "status 4" if res.status == brlen_ref.BRACKET else "the tolerance test ends it"))
        if res.status == brlen_ref.CAP:
            keys.add(("cap",))
        for k in keys:
            count[k] = count.get(k, 0) + 1
    print({k: count[k] for k in sorted(count, key=str)})
    need = [("status", s) for s in range(6)] + [("root", "both"), ("root", "band"), ("root", "kept"), ("u - v >= DBL_MIN", "status 4"),
                                               ("u - v >= DBL_MIN", "the tolerance test ends it"), ("cap",)]
    need += [("family", k) for k in ("unimodal", "oscillating", "inconsistent", "zeros", "holes", "tiny", "flat")]
    assert all(count.get(k, 0) >= AT_LEAST for k in need), {k: count.get(k, 0) for k in need}


def test_the_header_takes_the_restatements_steps(searches, tmp_path):
    assert len(searches) >= 20000
    got = _run_c(tmp_path, [_item(args, res) for _, args, res in searches])
    differ = 0
    for (kind, args, res), g in zip(searches, got):
        try:
            _assert_equal((kind, args), res, g)
        except AssertionError as e:
            differ += 1
            if differ <= 5:
                print(e)
    print(len(searches), "searches,", differ, "differ")
    assert differ == 0


def _one(dlk, *args):
    return args, brlen_ref.br_len_spline(dlk, *args)


def test_a_zero_start_with_a_nan_derivative(tmp_path):
    """l0 = 0.0 and a NaN derivative at the first probe: neither walk moves, u = l_min, v = the unclamped start 0.0, every root is
    NaN, and :2372's u / v is l_min / 0.0 = +inf > 1.1 in C -- the assert, status 3 after one evaluation.  (The restatement once
    answered nan for any v == 0 and went on to probe new_l = -1.)  0 / 0 is NaN in C too: neither comparison holds, new_l is kept."""
    args, res = _one(lambda l: (max(l, 1e-8), -100.0, NAN), 0.0, -100.0, 1e-8, 100.0, 1000, 1e-3, brlen_ref.trip_cap(1e-8, 100.0))
    assert (res.status, res.evaluations, res.l) == (brlen_ref.NO_ROOT, 1, 0.0)
    assert brlen_ref.pick_root(1e-8, 0.0, NAN, NAN) == (-1, None) and brlen_ref.pick_root(-1e-8, 0.0, NAN, NAN) == (-1, None)
    assert brlen_ref.pick_root(0.0, 0.0, NAN, NAN) == (0, None)
    _assert_equal("l0 = 0, NaN derivative", res, _run_c(tmp_path, [_item(args, res)])[0])


def test_a_nan_start_is_status_6(tmp_path):
    args, res = _one(lambda l: (l, -1.0, 1.0), NAN, -5.0, 1e-8, 100.0, 1000, 1e-3, 50)
    assert (res.status, res.evaluations, res.probes) == (brlen_ref.NAN, 0, []) and res.l != res.l and (res.lnL, res.dlnL) == (-5.0, 0.0)
    _assert_equal("NaN start", res, _run_c(tmp_path, [_item(args, res)])[0])


@pytest.mark.parametrize("cap", [0, 1, 5])
def test_the_trip_cap_is_status_7(tmp_path, cap):
    """between l_min and l_max the cap of the device call never binds; a small one handed to both sides does, in either walk"""
    items, results = [], []
    for slope in (-1e-3, 1e-3):
        dlk = lambda l, slope=slope: (min(max(l, 1e-8), 100.0), -50.0 + slope * min(max(l, 1e-8), 100.0), slope)
        args, res = _one(dlk, 0.1, -50.0, 1e-8, 100.0, 1000, 1e-3, cap)
        assert (res.status, res.evaluations, res.n_tot) == (brlen_ref.CAP, 1 + cap, 1 + cap), (slope, res.status, res.evaluations)
        full = brlen_ref.br_len_spline(dlk, 0.1, -50.0, 1e-8, 100.0)
        assert full.status in (brlen_ref.LOWER, brlen_ref.UPPER) and full.evaluations < brlen_ref.trip_cap(1e-8, 100.0)
        items.append(_item(args, res)); results.append(res)
    for res, g in zip(results, _run_c(tmp_path, items)):
        _assert_equal(("cap", cap), res, g)


def test_too_few_and_too_many_responses_are_reported(tmp_path):
    """the program says so where the responses it is given are not the ones it needs (the harness cannot agree by running short)"""
    dlk = lambda l: (min(max(l, 1e-8), 100.0), -3.0 * (min(max(l, 1e-8), 100.0) - 0.3) ** 2, -6.0 * (min(max(l, 1e-8), 100.0) - 0.3))
    args, res = _one(dlk, 0.05, -1.0, 1e-8, 100.0, 1000, 1e-3, 100)
    resp = [(p[1], p[2]) for p in res.probes]
    assert res.status == 0 and len(resp) >= 3
    short, exact, long_ = _run_c(tmp_path, [_item(args, res, resp[:-1]), _item(args, res), _item(args, res, resp + [(0.0, 0.0)])])
    assert (short[6], short[7]) == (len(resp), len(resp) - 1)
    assert (exact[6], exact[7]) == (len(resp), len(resp))
    assert (long_[6], long_[7]) == (len(resp), len(resp) + 1)
