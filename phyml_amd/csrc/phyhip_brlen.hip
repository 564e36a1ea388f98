// phyhip_brlen.hip -- one edge's branch-length search in one device call: phyhip_optimise_edge_length
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// Br_Len_Opt (src/optimiz.c:607-663) optimises one edge with Br_Len_Spline (src/optimiz.c:2244-2470): dLk at the start length, a walk
// down in factors of 1.2 until the first derivative is positive, a walk up from the start until it is negative, then a root of the
// cubic spline through the two bracket ends.  Every probe is one dLk (src/lk.c:655-753) on the SAME eigen-basis products: driven
// from the host it is one round trip per probe whose only use is to choose the next probe, and a near-zero branch takes 30-110 of
// them.  Here the whole search is ONE plain launch of ONE workgroup:
//   * brlen_opt_kernel<S, CP>, grid 1, kBrlenThreads<S> threads.  Lane gl of round r holds (pattern, category) gl = thread + r * threads,
//     as dlk_kernel's lanes do.  The products and the three per-pattern scalars of a lane's first kBrlenKeep<S> rounds are fetched
//     ONCE and stay in registers across evaluations (DlkIn<S>, as dlk_tile keeps them); rounds beyond are fetched again by every
//     evaluation and come from the L2.
//   * one evaluation is dLk's body: the clamp of l, the expl table built in LDS (dlk_expl_from_len), dlk_lane per (pattern,
//     category) -- the same per-pattern doubles as every other shape of the evaluation -- and the two sums in one fixed order: a
//     lane's rounds in ascending order, the wave's shuffle-down tree 32..1, then thread 0 adds the waves in wave order.
//   * the search is Br_Len_Spline line by line (brlen_step: what it does, not what it seems to mean).  Thread 0 takes its steps on
//     a state that lives in LDS and leaves the next probe's length, or the end, there: every thread reads the same two words, so
//     the control flow is uniform over the workgroup and no register holds search state while the workgroup evaluates.  The
//     reference's asserts and early returns become a status word (include/phyhip.h).  Every loop has a trip count bounded by the
//     host; nothing waits for anything but __syncthreads and the kernel's own loads; no polling, nothing resident, no
//     read-modify-write atomic (the one atomic operation is dlk_lane's own raise_warn, a store, aimed here at a flag in LDS).
// The kernel writes one record {l, lnL, dlnL, evaluations, status, warning} into host-mapped memory and nothing else; the host
// reads it once the stream has drained.  Partials, matrices, site outputs, dot_prod and the queue stay what they were; the numerical
// warning becomes that of the search's last evaluation.
#include "phyhip_side.hpp"
#include "phyhip_brlen_step.h"

namespace phyhip_host
{

// The one workgroup: 16 waves at 4 states (four per SIMD: 128 registers each at most), 8 at 20 states (two per SIMD, 256 each:
// dlk_lane's working set at 20 states is about 160 registers by itself).  Compiled with -disable-machine-licm (__graft_entry__.py):
// hoisting the probe loop's invariants costs the registers that the kept rounds are for.
template <int S> constexpr int kBrlenThreads = S == 4 ? 1024 : 512;
template <int S> constexpr int kBrlenKeep = S == 4 ? 3 : 1; // rounds whose inputs stay in registers (about 15 VGPRs a round at 4 states, 44 at 20)
constexpr long long kBrlenMaxPatterns = 16384;         // above, the host-driven chain of launched dLk calls wins (profiles/brlen_opt.md)
constexpr int       kBrentItMax = 1000;                // BRENT_IT_MAX, src/utilities.h:337


struct BrlenResult
{
  double l, lnl, dlnl;
  int    evaluations, status, warning, pad;
};

// (the kernel arguments hold 4 KiB: DlkParams is what dlk_fetch / dlk_lane read, passed whole)
struct BrlenParams
{
  DlkParams    q; // (expl, fin, from_len, len: not used -- the table is built in LDS from the length of each probe)
  double       l0, init_lnl, tol;
  int          n_iter_max, cap; // (cap: brlen_trip_cap, the bound of both bracket walks)
  BrlenResult *out;
};

static_assert(sizeof(BrlenParams) <= 4096, "kernel arguments");

template <int S, int CP>
__global__ __launch_bounds__(kBrlenThreads<S>) void brlen_opt_kernel(const BrlenParams a)
{
  constexpr int R = kBrlenKeep<S>, W = kBrlenThreads<S>, NW = W / 64;
  __shared__ double     sh_tab[kMaxExpl];
  __shared__ double     sh_ws[2][NW];
  __shared__ int        sh_warn;
  __shared__ BrlenState st;
  const DlkParams &q = a.q;
  const DlkCall   k = {1, q.invar_model, q.apply_scaling, q.pinvar};
  const int       tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int       total = (((int)q.P * CP + 255) / 256) * 256; // (dlk_block's: whole waves are in or out of a round; P <= kBrlenMaxPatterns)

  DlkIn<S> in[R];
#pragma unroll
  for (int u = 0; u < R; ++u)
    if (tid + u * W < total) dlk_fetch<S, CP>(q, k, tid + u * W, in[u]);

  if (tid == 0)
  {
    brlen_begin(&st, a.l0, a.init_lnl, a.tol, q.l_min, q.l_max, a.n_iter_max, a.cap);
    sh_warn   = 0; // :669
  }
  __syncthreads();

  // every probe ends the loop or names the next one; the walks and the spline loop are bounded by the caps and n_iter_max + 20
  while (!st.done)
  {
    // ---- dLk(l), src/lk.c:655-753
    double l = st.l;
    if (l < q.l_min) l = q.l_min; // :673-674: the clamped value is what the search keeps
    else if (l > q.l_max) l = q.l_max;
    dlk_expl_from_len<S>(sh_tab, l, true, q.C, q.eval_dev, q.rates_dev, q.br_len_mult, q.l_min, q.l_max, tid, W);
    __syncthreads();
    double t_lnl = 0.0, t_dlnl = 0.0;
#pragma unroll
    for (int u = 0; u < R; ++u)
    {
      const int gl = tid + u * W;
      if (gl < total)
      {
        double c0, c1;
        dlk_lane<S, CP>(q, k, sh_tab, &sh_warn, gl, in[u], c0, c1);
        t_lnl += c0;
        t_dlnl += c1;
      }
      __builtin_amdgcn_sched_barrier(0); // (one round's working set at a time: the rounds' inputs are what the registers are for)
    }
#pragma unroll 1
    for (int gl = tid + R * W; gl < total; gl += W)
    {
      DlkIn<S> x;
      dlk_fetch<S, CP>(q, k, gl, x);
      double c0, c1;
      dlk_lane<S, CP>(q, k, sh_tab, &sh_warn, gl, x, c0, c1);
      t_lnl += c0;
      t_dlnl += c1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
      t_lnl += __shfl_down(t_lnl, off, 64);
      t_dlnl += __shfl_down(t_dlnl, off, 64);
    }
    if (lane == 0)
    {
      sh_ws[0][wid] = t_lnl;
      sh_ws[1][wid] = t_dlnl;
    }
    __syncthreads();
    if (tid == 0)
    {
      double s0 = 0.0, s1 = 0.0;
      for (int w = 0; w < NW; ++w)
      {
        s0 += sh_ws[0][w];
        s1 += sh_ws[1][w];
      }
      st.l = l;
      brlen_step(&st, s0, s1, sh_warn);
      sh_warn = 0; // :669, for the next probe
    }
    __syncthreads(); // (the next probe's length and whether there is one; it rewrites the table and the waves' sums)
  }

  if (tid == 0)
  { // :2460-2461: *l = best_l, c_lnL = best_lnL; c_dlnL and the warning are the last evaluation's
    BrlenResult r;
    r.l = st.best_l; r.lnl = st.best_lnL; r.dlnl = st.c_dlnL;
    r.evaluations = st.evals; r.status = st.status; r.warning = st.warn; r.pad = 0;
    *a.out = r;
  }
}

static int brlen_run(Instance *I, double *l, double initLnL, int iterMax, double tol, BrlenResult &res)
{
  static const char *const who = "phyhip_optimise_edge_length";
  int rc = refuse_kind(I, who, kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop | kRefuseStates);
  if (rc) return rc;
  if (I->NE != 1) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d eigen systems", who, I->NE);
  if (I->C < 1 || I->C > 8) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d categories", who, I->C);
  long long max_patterns = kBrlenMaxPatterns;
  if (const char *e = diag_env("PHYHIP_BRLEN_MAX_PATTERNS")) max_patterns = std::min(std::max(1ll, atoll(e)), 1ll << 24); // (the timing sweep)
  if (I->P > max_patterns)
    return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for more than %lld patterns (%lld): drive phyhip_calculate_eigen_lnl_dlnl", who,
                max_patterns, I->P);
  if (std::isnan(*l) || std::isnan(initLnL)) return fail(PHYHIP_ERROR_FLOATING_POINT, "%s: branch length or initLnL is NaN", who);
  if (iterMax < 1 || iterMax > kBrentItMax) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "iterMax %d (1..%d)", iterMax, kBrentItMax);
  if (!(tol > 0.0)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "tol %g (must be > 0)", tol);

  auto &U = side_of(I).brlen;
  if (!U.h_out) HIPCHK(hipHostMalloc((void **)&U.h_out, sizeof(BrlenResult), hipHostMallocMapped));
  // what eigen_eval does in front of a launched dlk_kernel: the queue, then the launch on the instance's stream
  if ((rc = flush(I, nullptr))) return rc;

  BrlenParams a;
  memset(&a, 0, sizeof a);
  DlkParams &q = a.q;
  q.dot_prod = I->d_dot; q.wght = I->d_wght; q.fact = I->d_fact; q.cat_w = I->d_catw; q.pi = I->d_pi; q.invar = I->d_invar;
  q.P = I->P; q.C = I->C; q.invar_model = I->invar_model; q.apply_scaling = I->apply_scaling; q.with_derivative = 1; q.pinvar = I->pinvar;
  q.eval_dev = I->d_eval; q.rates_dev = I->d_catr; q.br_len_mult = I->br_len_mult; q.l_min = I->l_min; q.l_max = I->l_max;
  a.l0 = *l; a.init_lnl = initLnL; a.tol = tol; a.n_iter_max = iterMax;
  a.out = (BrlenResult *)U.h_out;
  a.cap = brlen_trip_cap(I->l_min, I->l_max);

  BrlenResult *const h = (BrlenResult *)U.h_out;
  h->status = -1;
  SideTimer tm(I);
  if ((rc = tm.tic())) return rc;
  rc = dispatch_shape(I, [&](auto s, auto cp) {
    constexpr int S_ = decltype(s)::value, CP_ = decltype(cp)::value;
    if constexpr (CP_ <= 8) hipLaunchKernelGGL((brlen_opt_kernel<S_, CP_>), dim3(1), dim3(kBrlenThreads<S_>), 0, I->stream, a);
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  if ((rc = tm.mark())) return rc;
  HIPCHK(hipStreamSynchronize(I->stream)); // (the record is in host memory once the kernel has ended)
  if ((rc = tm.toc(U.prof_ms))) return rc;
  side_stream_drained(I); // the dLk calls that follow can be served resident again
  if (h->status < 0) return fail(PHYHIP_ERROR_GENERAL, "%s: the search finished without handing its result over", who);
  res = *h;
  if (I->prof)
  {
    ++U.prof_n;
    U.prof_evals += res.evaluations;
  }
  // the stream is idle: the flag the host reads (phyhip_get_numerical_warning) is the last evaluation's
  *I->h_warn      = res.warning;
  I->warn_current = true;
  *l = res.l;
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

int phyhip_optimise_edge_length(int instance, double *l, double initLnL, int iterMax, double tol, double *outLnL, double *outDLnL,
                                int *outEvaluations, int *outStatus)
{
  if (!l) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_optimise_edge_length: l is NULL");
  if (get_group(instance))
    return fail(PHYHIP_ERROR_NO_IMPLEMENTATION,
                "phyhip_optimise_edge_length: not built for one-process sharded instances (each probe needs every shard's sums)");
  GET_INST(I, instance);
  BrlenResult r;
  const int rc = brlen_run(I, l, initLnL, iterMax, tol, r);
  if (rc) return rc;
  if (outLnL) *outLnL = r.lnl;
  if (outDLnL) *outDLnL = r.dlnl;
  if (outEvaluations) *outEvaluations = r.evaluations;
  if (outStatus) *outStatus = r.status;
  return PHYHIP_SUCCESS;
}

int phyhip_profile_read_edge_length(int instance, double *outKernelMs, int *outCalls, long long *outEvaluations)
{
  double    ms = 0.0;
  int       n = 0;
  long long ev = 0;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).brlen;
    ms += U.prof_ms;
    n += U.prof_n;
    ev += U.prof_evals;
    U.prof_ms = 0.0;
    U.prof_n = 0;
    U.prof_evals = 0;
    return 0;
  });
  if (rc < 0) return rc;
  if (outKernelMs) *outKernelMs = ms;
  if (outCalls) *outCalls = n;
  if (outEvaluations) *outEvaluations = ev;
  return PHYHIP_SUCCESS;
}

} // extern "C"
