/* phyhip_brlen_step.h -- Br_Len_Spline (src/optimiz.c:2244-2470) from one dLk to the next: the ONE statement of the search's control
   flow.  The search kernel of phyhip_optimise_edge_length compiles it for the device (phyhip_brlen.hip: thread 0 takes the steps on
   a state in LDS) and the host layer's Br_Len_Opt compiles it for the host (host/phl_lk.c: the same steps driving dLk(), one round
   trip per probe), so the two routes cannot drift apart.  Plain C that is also C++ and HIP; tests/brlen_ref.py is its restatement
   for the tests.  What it does, not what it seems to mean: init_lnL is the caller's matrix-route c_lnL; best_l starts as the
   unclamped start and the upper walk restarts from it; the two resets sit behind a dLk that has clamped; u - v < DBL_MIN ends the
   loop after one step; new_l keeps -1. when no root is accepted. */
#ifndef PHYHIP_BRLEN_STEP_H
#define PHYHIP_BRLEN_STEP_H
#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define PHYHIP_BRLEN_FN __host__ __device__ __forceinline__
#else
#define PHYHIP_BRLEN_FN static inline
#endif

/* the status word of phyhip_optimise_edge_length (include/phyhip.h) */
enum { kBrlenSpline = 0, kBrlenLower = 1, kBrlenUpper = 2, kBrlenNoRoot = 3, kBrlenBracket = 4, kBrlenTooLong = 5, kBrlenNaN = 6, kBrlenCap = 7 };
#define PHYHIP_BRLEN_TRIP_MAX 8192 /* no bracket walk is allowed more trips than this */

// What Br_Len_Spline keeps from one probe to the next.  It lives in LDS: thread 0 alone takes the search's steps, so that no register
// holds any of it while the workgroup evaluates (the inputs kept in registers and dlk_lane's working set have the budget to themselves)
typedef struct BrlenState
{
  double l;                                    // *l: the length of the next probe; clamped by it
  double init_dl, best_l, best_lnL, old_lnL;
  double c_lnL, c_dlnL;                        // tree->c_lnL, tree->c_dlnL
  double u, v, fu, fv, dfu, dfv, new_l;
  int    evals, status, iter, trips, phase, warn, done;
  // the call's own scalars, copied here once (read by thread 0 alone: they need not occupy scalar registers during the probes)
  double init_l, init_lnL, tol, l_min, l_max;
  int    n_iter_max, cap_lower, cap_upper;
} BrlenState;

// Br_Len_Spline, src/optimiz.c:2244-2470, from one dLk to the next: the probe at s.l has given (lnL, dlnL, warn).  There is one
// call site of the evaluation, so the probe in front of the loops (phase 0), the ones of the lower (1) and upper (2) bracket walk
// and the spline's (3) take turns.  Sets s.l for the next probe, or s.done.
PHYHIP_BRLEN_FN void brlen_step(BrlenState *sp, const double lnL, const double dlnL, const int warn)
{
#define s (*sp)
#define a (*sp)
  const double l_min = s.l_min, l_max = s.l_max, mult = 1.2, init_l = s.init_l, init_lnL = s.init_lnL;
  s.c_lnL  = lnL; // src/lk.c:749-750
  s.c_dlnL = dlnL;
  s.warn   = warn;
  ++s.evals;
  if (s.phase == 0)
  {
    s.init_dl = dlnL;                // :2269
    if (s.l > l_max) s.l = 0.5;      // :2271-2272, behind a dLk that has already clamped
    if (s.l < l_min) s.l = 0.001;
    s.phase = 1;
    s.trips = 0;
  }
  else
  {
    if (lnL > s.best_lnL) // :2287-2291, :2315-2319, :2384-2388
    {
      s.best_lnL = lnL;
      s.best_l   = s.l;
    }
    if (s.phase == 3)
    {
      if (dlnL > 0.0) // :2390-2401
      {
        s.u = s.new_l; s.fu = lnL; s.dfu = dlnL;
      }
      else
      {
        s.v = s.new_l; s.fv = lnL; s.dfv = dlnL;
      }
      int converged = 0;
      if (s.u - s.v < DBL_MIN) converged = 1; // :2405 (true whenever u < v)
      if (fabs(lnL - s.old_lnL) < a.tol) converged = 1;
      if (++s.iter == a.n_iter_max + 20) converged = 1;
      if (converged)
      {
        s.status = s.iter == a.n_iter_max ? kBrlenTooLong : kBrlenSpline; // :2463
        s.done   = 1;
        return;
      }
      if (!(s.u < s.v) || !(s.dfu > 0.0) || !(s.dfv < 0.0)) // :2423-2425
      {
        s.status = kBrlenBracket;
        s.done   = 1;
        return;
      }
    }
  }
  if (s.phase == 1)
  { // the lower walk, :2274-2295: down in factors of 1.2 until the derivative is not negative any more
    if (s.c_dlnL < 0.0)
    {
      s.l = s.l / mult;
      if (s.l < l_min) // :2280-2285
      {
        s.status = kBrlenLower;
        s.done   = 1;
      }
      else if (s.trips++ >= a.cap_lower)
      {
        s.status = kBrlenCap;
        s.done   = 1;
      }
      return;
    }
    s.u = s.l; s.fu = s.c_lnL; s.dfu = s.c_dlnL;
    s.l = init_l; s.c_dlnL = s.init_dl; s.c_lnL = init_lnL; // :2300-2302
    s.phase = 2;
    s.trips = 0;
  }
  if (s.phase == 2)
  { // the upper walk, :2304-2323: up from the caller's start until the derivative is not positive any more
    if (s.c_dlnL > 0.0)
    {
      s.l = s.l * mult;
      if (s.l > l_max) // :2308-2313
      {
        s.status = kBrlenUpper;
        s.done   = 1;
      }
      else if (s.trips++ >= a.cap_upper)
      {
        s.status = kBrlenCap;
        s.done   = 1;
      }
      return;
    }
    s.v = s.l; s.fv = s.c_lnL; s.dfv = s.c_dlnL;
    s.phase = 3;
    s.iter  = 0;
  }
  // the cubic through (u, fu, dfu) and (v, fv, dfv) and the zeros of its derivative, :2344-2383
  const double u = s.u, v = s.v, fu = s.fu, fv = s.fv, dfu = s.dfu, dfv = s.dfv;
  const double ha = dfu * (v - u) - (fv - fu);
  const double hb = -dfv * (v - u) + (fv - fu);
  const double q2 = 3. * ha - 3. * hb;
  const double q1 = -4. * ha + 2. * hb;
  const double q0 = fv - fu + ha;
  const double rt = sqrt(q1 * q1 - 4. * q2 * q0);
  double       root1 = (-q1 - rt) / (2. * q2);
  double       root2 = (-q1 + rt) / (2. * q2);
  root1 = root1 * (v - u) + u;
  root2 = root2 * (v - u) + u;
  int ok1 = 0, ok2 = 0;
  if (root1 > u && root1 < v) ok1 = 1;
  if (root2 > u && root2 < v) ok2 = 1;
  if (fabs(root1 - u) < 1.E-5) ok1 = 1; // Are_Equal, src/utilities.c:10982
  if (fabs(root2 - u) < 1.E-5) ok2 = 1;
  if (fabs(root1 - v) < 1.E-5) ok1 = 1;
  if (fabs(root2 - v) < 1.E-5) ok2 = 1;
  if (ok1 && ok2) s.new_l = root1 < root2 ? root1 : root2;
  else if (ok1) s.new_l = root1;
  else if (ok2) s.new_l = root2;
  else if (u / v > 1.1 || u / v < 0.9) // :2372-2376 (else new_l keeps what it was: -1. at first)
  {
    s.status = kBrlenNoRoot;
    s.done   = 1;
    return;
  }
  s.l       = s.new_l;
  s.old_lnL = s.c_lnL;
  if (s.l != s.l) // src/lk.c:671
  {
    s.status = kBrlenNaN;
    s.done   = 1;
  }
#undef s
#undef a
}

/* the trips a walk in factors of 1.2 can take between l_min and l_max (a probe clamps *l where it stands, so a walk that restarts
   from a length below l_min goes on from l_min): the bound of both walks, computed on the host */
static inline int brlen_trip_cap(double l_min, double l_max)
{
  const double span = log(l_max / l_min) / log(1.2);
  if (!(span > 0.0) || isinf(span)) return 2;
  return ceil(span) + 2.0 > (double)PHYHIP_BRLEN_TRIP_MAX ? PHYHIP_BRLEN_TRIP_MAX : (int)(ceil(span) + 2.0);
}

/* :2260-2266 (tree->c_lnL is the CALLER's: the matrix route's) */
PHYHIP_BRLEN_FN void brlen_begin(BrlenState *st, double l0, double init_lnL, double tol, double l_min, double l_max, int n_iter_max, int cap)
{
  st->init_l = l0; st->init_lnL = init_lnL; st->tol = tol; st->l_min = l_min; st->l_max = l_max;
  st->n_iter_max = n_iter_max; st->cap_lower = st->cap_upper = cap;
  st->l = l0;
  st->best_l = l0; st->best_lnL = st->old_lnL = st->c_lnL = init_lnL;
  st->init_dl = st->c_dlnL = 0.0;
  st->u = st->v = st->fu = st->fv = st->dfu = st->dfv = st->new_l = -1.;
  st->evals = st->iter = st->trips = st->phase = st->warn = 0;
  st->status = l0 != l0 ? kBrlenNaN : kBrlenSpline; /* src/lk.c:671 */
  st->done   = l0 != l0 ? 1 : 0;
}
#endif
