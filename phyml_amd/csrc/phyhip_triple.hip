// phyhip_triple.hip -- Triple_Dist at K nodes in one device call: phyhip_optimise_triples
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// Triple_Dist (src/utilities.c:7120-7146) optimises the three edges of a node a one after the other: Update_Partial_Lk(a->b[i], a),
// Br_Len_Opt(a->b[i]) for i = 0, 1, 2, then the partials of b[1] and b[0] once more.  Br_Len_Opt (src/optimiz.c:607-663) is Lk(b)
// with update_eigen_lr, Br_Len_Spline on the edge's eigen-basis products, and the matrix refresh.  Driven from the host that is five
// partial updates, three Lk(b) and 6-330 dLk probes per node, each a round trip whose only use is to choose the next one -- and
// none of it touches anything but the node's three OUTER vectors (the ones that look at a along its edges), which never change.  So
// the K nodes of a list are independent, and here each has ONE workgroup of ONE plain launch:
//   triple_kernel<S, CP, L>, grid K, kTripleThreads<S> threads.  A candidate's chain, all of it inside its workgroup:
//     * the three matrices: regraft_pmat_body per (edge, category), PMat_Empirical as every device-built matrix has it, into the
//       candidate's own area of the work space -- the instance's matrix table is neither read nor written;
//     * I_i, one lane per pattern (pattern = thread + round * threads): regraft_join's vector with the scaling decision found in a
//       first pass over the categories and applied in a second (the form regraft_scan_kernel takes at 20 states, here at both: the
//       same doubles, and C * S values of a lane do not have to wait in registers); the matrices are read from LDS: at 4 states all
//       categories' are staged once per step (3 KiB) and the pattern rounds run without a barrier, at 20 states one category's at
//       a time, staged by the workgroup in every round;
//     * in that second pass, category by category: regraft_product through matrix i -- Lk_Core's per-category term of lk_begin --
//       and the S eigen-basis products of (pattern, category), eigen_lr_kernel's arithmetic (first product, then the FMA chains;
//       the LEFT operand is the one multiplied by pi), stored to the candidate's products [pattern][category][state];
//     * the shared site tail (phyhip_tail.hpp: fused +I mix, the ported log) gives the pattern's term of lk_begin and its exponent
//       (stored for the probes); lk_begin is summed in one fixed order: a lane's rounds in ascending order, the wave's shuffle-down
//       tree 32..1, thread 0 adds the waves in wave order;
//     * the search: brlen_opt_kernel's loop -- lane gl = (pattern, category) as dlk_kernel's lanes, the first kTripleKeep<S> rounds
//       of a lane fetched once, dlk_expl_from_len, dlk_lane, the two sums in the same fixed order, brlen_step by thread 0 on a
//       state in LDS;
//     * length[i] = best_l, matrix i rebuilt, Br_Len_Opt's lk_end check (status 8).
//     A status of 3..8 ends the candidate.  The kept candidate then rebuilds I_1 and I_0; its I_i go to the kept area instead of
//     nowhere (no other candidate's vector is ever stored).
// A pattern's work never leaves its workgroup: __syncthreads is the only synchronisation.  Nothing is resident, nothing polls, no
// read-modify-write atomic (dlk_lane's raise_warn is a store, aimed at a flag in LDS); every loop's trip count is bounded by the
// host (the pattern rounds, brlen_step's caps and iterMax + 20).  The result record of a candidate is written by thread 0 with
// ordinary stores into the work space and copied down after the stream has drained.  Its bits depend on the candidate alone: the
// workgroup reads nothing another candidate writes, and its geometry does not depend on K or on the chunking.
// Compiled with -disable-machine-licm, for brlen_opt_kernel's reason: hoisting the probe loop's invariants costs the registers
// that the kept rounds are for.
#include "phyhip_regraft_dev.hpp"
#include "phyhip_scan.hpp" // the chunk walk; the work-space layout: phyhip_scan_plan.hpp
#include "phyhip_brlen_step.h"

namespace phyhip_host
{

// The workgroup is half of brlen_opt_kernel's: the lane-per-pattern passes hold two operands, the joined vector and the outer vector
// of a (pattern, category) at once -- 4 S doubles -- and take 256 registers a lane at 4 states, 512 at 20 (two waves / one wave per
// SIMD); and a list of K candidates fills the device with K workgroups where one search had a single one to show.  The search keeps
// the inputs of 2 560 lanes in registers at 4 states (five rounds: with a sixth -- brlen_opt_kernel's 3 072 lanes -- the kernel spilled
// seven vector registers) and of 512 at 20, as brlen_opt_kernel does.
template <int S> constexpr int kTripleThreads = S == 4 ? 512 : 256;
template <int S> constexpr int kTripleKeep = S == 4 ? 5 : 2; // rounds of the search whose inputs stay in registers (about 15 VGPRs a round at 4 states, 44 at 20)
constexpr long long kTripleMaxPatterns = 16384;
constexpr int       kTripleMaxCategories = 8;
constexpr int       kTripleIterMax = 1000;                           // BRENT_IT_MAX, src/utilities.h:337
constexpr int       kTripleLkEnd = 8;                                // status: lk_end < lk_begin - tol, src/optimiz.c:656

static_assert(sizeof(phyhip_triple_candidate) == 40 && sizeof(phyhip_triple_result) == 96, "the records of include/phyhip.h");

struct TripleParams
{
  DlkParams                      q; // what dlk_lane reads (dot_prod, fact, expl, fin, from_len, len: not used -- they are per candidate)
  const uint8_t                 *tip_codes;
  const uint32_t                *code_masks;
  const double                  *partials;
  const int                     *scales;
  const double                  *U, *V, *R; // the eigen system: right and left eigenvectors, eigenvalues
  const phyhip_triple_candidate *recs;      // [candidate of the launch]
  phyhip_triple_result          *out;       // [candidate of the launch]
  double                        *mats;      // [candidate][3][C][S][S]
  double                        *dot;       // [candidate][P][C][S]
  int                           *fact;      // [candidate][Pe]
  double                        *keep;      // [3][P][C][S], host order; behind them their exponents, [3][Pe] ints
  long long                      Ppad, Pe;  // (Pe: P rounded up to even)
  int                            tips, keep_cand;
  double                         tol;
  int                            n_iter_max, cap;
};
static_assert(sizeof(TripleParams) <= 4096, "kernel arguments");

// the exponent is the one output of the tail that is kept
struct TripleFactStore
{
  __device__ __forceinline__ void operator()(double *, const double) const {}
  __device__ __forceinline__ void operator()(int *ptr, const int v) const { *ptr = v; }
};

// dlk_fetch on a candidate's own products and exponents
template <int S, int CP>
__device__ __forceinline__ void triple_fetch(const DlkParams &q, const DlkCall &k, const double *__restrict__ dot, const int *__restrict__ fact,
                                             const int gl, DlkIn<S> &in)
{
  const int p0 = gl / CP, c0 = gl % CP;
  const int p = (p0 < (int)q.P) ? p0 : ((int)q.P - 1);
  const int c = (c0 < q.C) ? c0 : 0;
  in.wt = q.wght[p];
  in.f  = fact[p];
  in.iv = k.invar_model ? (int)q.invar[p] : -1;
  const double2 *s2 = reinterpret_cast<const double2 *>(dot + (size_t)p * (q.C * S) + (size_t)c * S);
#pragma unroll
  for (int j = 0; j < S / 2; ++j) in.d[j] = s2[j];
}

template <int S, int CP, int L>
__global__ __launch_bounds__(kTripleThreads<S>) void triple_kernel(const TripleParams a)
{
  constexpr int SS = S * S, R = kTripleKeep<S>, W = kTripleThreads<S>, NW = W / 64;
  constexpr int MC = S == 4 ? kTripleMaxCategories : 1; // categories whose three matrices LDS holds at a time: all of them at 4 states (3 KiB)
  // regraft_pmat_body strides by 256: every entry of a matrix is written, and written once, where S * S <= 256 or the workgroup has 256 threads
  static_assert(SS <= 256 || W == 256, "regraft_pmat_body's stride");
  __shared__ double               sh_tab[kMaxExpl];
  __shared__ double               sh_ws[2][NW];
  __shared__ double               Ms[3 * MC * SS], Ev[2 * SS], pis[S], p_expt[S], p_tmp[SS], p_rsum[S], sh_len[3];
  __shared__ int                  sh_warn, sh_stop;
  __shared__ BrlenState           st;
  __shared__ phyhip_triple_result res;
  const DlkParams &q = a.q;
  const DlkCall   k = {1, q.invar_model, q.apply_scaling, q.pinvar};
  const int       tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int       cand = blockIdx.x, P = (int)q.P, C = q.C;
  const size_t    CS = (size_t)C * S;
  const phyhip_triple_candidate *rec = a.recs + cand;
  double *const   mats = a.mats + (size_t)cand * 3 * C * SS;
  double *const   dot = a.dot + (size_t)cand * P * CS;
  int *const      fact = a.fact + (size_t)cand * a.Pe;
  const bool      keep = a.keep_cand == cand;
  const int       flags = rec->flags;
  const int       total = ((P * CP + 255) / 256) * 256; // (dlk_block's: whole waves are in or out of a round)
  const int       rounds = (P + W - 1) / W;             // ... and of the lane-per-pattern passes
  const MixRegraftSrc src{a.partials, q.P, a.Ppad, C, a.tips};

  for (int t = tid; t < SS; t += W)
  {
    Ev[t]      = a.U[t];
    Ev[SS + t] = a.V[t];
  }
  if (tid < S) pis[tid] = q.pi[tid];
  if (tid < 3) sh_len[tid] = rec->length[tid];
  if (tid == 0)
  {
    for (int i = 0; i < 3; ++i)
    {
      res.length[i] = rec->length[i]; res.lkBegin[i] = 0.0; res.evaluations[i] = 0; res.status[i] = -1;
    }
    res.lnL = res.dLnL = 0.0; res.warning = 0; res.reserved = 0;
    sh_warn = 0; sh_stop = 0;
  }
  __syncthreads();
  // matrix m of the current lengths, category by category (the workgroup's next barrier makes it visible to all of its lanes)
  auto build_matrix = [&](const int m) {
    for (int c = 0; c < C; ++c)
      regraft_pmat_body<S>(sh_len[m], Ev, Ev + SS, a.R, q.rates_dev[c], q.br_len_mult, q.l_min, q.l_max, mats + ((size_t)m * C + c) * SS, p_expt, p_tmp,
                           p_rsum);
  };
  for (int m = 0; m < 3; ++m) build_matrix(m);

  // steps 0..2: I_i, lk_begin, the products and the search of edge i; steps 3, 4 (the kept candidate alone): I_1 and I_0 again
  for (int step = 0; step < 5; ++step)
  {
    const bool eval = step < 3;
    if (!eval && !keep) break;
    const int  i = eval ? step : 4 - step;
    const int  j = i == 0 ? 1 : 0, kk = i == 2 ? 1 : 2; // the two other edges, ascending
    const bool node_left = ((flags >> i) & 1) != 0;
    RegraftRec r;
    r.c1 = rec->partials[j]; r.c2 = rec->partials[kk]; r.sub = rec->partials[i]; r.flags = 0; r.m1 = r.m2 = r.m3 = r.pad = 0;
    const double *const G1 = mats + (size_t)j * C * SS, *const G2 = mats + (size_t)kk * C * SS, *const G3 = mats + (size_t)i * C * SS;
    double *const kv = a.keep + (size_t)i * P * CS;
    int *const    ke = reinterpret_cast<int *>(a.keep + (size_t)3 * P * CS) + (size_t)i * a.Pe;
    if (tid == 0) sh_warn = 0;
    if constexpr (S == 4)
    { // the three matrices of every category, once per step: the pattern rounds below then need no barrier
      __syncthreads(); // (the matrices are in memory; the step before has read Ms)
      for (int t = tid; t < C * SS; t += W)
      {
        Ms[t]               = G1[t];
        Ms[MC * SS + t]     = G2[t];
        Ms[2 * MC * SS + t] = G3[t];
      }
      __syncthreads();
    }

    // (the thread index of this phase is opaque to the compiler: per-lane addresses that do not change from step to step would
    // otherwise be formed once in front of the step loop and wait in registers through the searches, which have none to spare)
    int jt = tid;
    asm volatile("" : "+v"(jt));
    double t_lnl = 0.0;
#pragma unroll 1
    for (int rd = 0; rd < rounds; ++rd)
    {
      const int    p = jt + rd * W;
      const bool   in = p < P;
      const double w = in ? q.wght[p] : 0.0;
      const bool   act = in && w > kSmall; // src/avx.c:399, src/lk.c:632
      uint32_t     k1 = 0, k2 = 0, k3 = 0;
      int          sc = 0, s3 = 0;
      if (act)
      {
        if (r.c1 < a.tips) k1 = tip_state_mask<S>(a.tip_codes, a.code_masks, a.Ppad, r.c1, p);
        else sc += a.scales[(size_t)(r.c1 - a.tips) * a.Ppad + p];
        if (r.c2 < a.tips) k2 = tip_state_mask<S>(a.tip_codes, a.code_masks, a.Ppad, r.c2, p);
        else sc += a.scales[(size_t)(r.c2 - a.tips) * a.Ppad + p]; // src/avx.c:462-464
        if (r.sub < a.tips) k3 = tip_state_mask<S>(a.tip_codes, a.code_masks, a.Ppad, r.sub, p);
        else s3 = a.scales[(size_t)(r.sub - a.tips) * a.Ppad + p];
      }
      // ---- pass 1: the largest of the C*S values (src/avx.c:497-502; `>`: a NaN never becomes the maximum)
      double mx = -__builtin_huge_val();
#pragma unroll 1
      for (int c = 0; c < C; ++c)
      {
        if constexpr (S != 4)
        { // 20 states: one category's matrices at a time, staged by the workgroup -- every lane takes part in the barriers
          __syncthreads();
          for (int t = jt; t < SS; t += W)
          {
            Ms[t]      = G1[c * SS + t];
            Ms[SS + t] = G2[c * SS + t];
          }
          __syncthreads();
        }
        if (!act) continue;
        double o[S];
        regraft_join<S, L>(src, r, k1, k2, p, c, Ms + (S == 4 ? c * SS : 0), Ms + (S == 4 ? (MC + c) * SS : SS), o);
#pragma unroll
        for (int s = 0; s < S; ++s) mx = (o[s] > mx) ? o[s] : mx;
      }
      const bool scale = act && mx < kInvTwoToLarge && q.apply_scaling; // src/avx.c:504-510
      if (scale) sc += kLarge;
      // ---- pass 2: the vector as stored; Lk_Core's product and the eigen-basis products with the outer vector of edge i
      double site = 0.0;
#pragma unroll 1
      for (int c = 0; c < C; ++c)
      {
        if constexpr (S != 4)
        {
          __syncthreads();
          for (int t = jt; t < SS; t += W)
          {
            Ms[t]          = G1[c * SS + t];
            Ms[SS + t]     = G2[c * SS + t];
            Ms[2 * SS + t] = G3[c * SS + t];
          }
          __syncthreads();
        }
        if (!act) continue;
        const double *const M3 = Ms + (S == 4 ? (2 * MC + c) * SS : 2 * SS);
        double o[S];
        regraft_join<S, L>(src, r, k1, k2, p, c, Ms + (S == 4 ? c * SS : 0), Ms + (S == 4 ? (MC + c) * SS : SS), o);
        if (scale)
        { // multiplication by 2^256 is exact
#pragma unroll
          for (int s = 0; s < S; ++s) o[s] *= kTwoToLarge;
        }
        if (keep)
        {
          double *__restrict__ dst = kv + ((size_t)p * C + c) * S;
#pragma unroll
          for (int s = 0; s < S; ++s) dst[s] = o[s];
        }
        if (!eval) continue;
        double y[S];
        regraft_operand<S, L>(src, r.sub, k3, p, c, y);
        const double lkc = regraft_product<S>(M3, o, y, pis, !node_left);
        site = site + lkc * q.cat_w[c]; // src/lk.c:818
        // Update_Eigen_Lr (src/avx.c:68-105): dot_prod[k] = (sum_s R[s][k] (x_s pi_s)) (sum_s L[k][s] y_s), x the LEFT side's vector
        double2 *__restrict__ dp = reinterpret_cast<double2 *>(dot + (size_t)p * CS + (size_t)c * S);
        double d0 = 0.0;
#pragma unroll
        for (int e = 0; e < S; ++e)
        {
          double ea = Ev[e] * ((node_left ? o[0] : y[0]) * pis[0]);
          double eb = Ev[SS + e * S] * (node_left ? y[0] : o[0]);
#pragma unroll
          for (int s = 1; s < S; ++s)
          {
            ea = __builtin_fma(Ev[s * S + e], (node_left ? o[s] : y[s]) * pis[s], ea);
            eb = __builtin_fma(Ev[SS + e * S + s], node_left ? y[s] : o[s], eb);
          }
          if (e & 1) dp[e >> 1] = make_double2(d0, ea * eb);
          else d0 = ea * eb;
        }
      }
      if (act)
      {
        if (keep) ke[p] = sc;
        if (eval)
        {
          RegraftTailQ tq;
          tq.invar = q.invar; tq.pi = q.pi; tq.site_lnl = nullptr; tq.site_lk = nullptr; tq.fact = fact; tq.warn = &sh_warn;
          tq.invar_model = q.invar_model; tq.apply_scaling = q.apply_scaling; tq.pinvar = q.pinvar;
          const int f = q.apply_scaling ? sc + s3 : 0; // Pull_Scaling_Factors, SCALE_FAST: src/lk.c:2701-2705, 2777-2801
          double    contrib = 0.0;
          site_tail<TailMix::fused, TailLibm::reference>(contrib, tq, (size_t)p, w, site, f, TripleFactStore());
          t_lnl += contrib;
        }
      }
      else if (in)
      { // a pattern without weight: no probe reads its products' sums, the reference leaves its entries of the vector as they were
        if (eval)
        {
          fact[p] = 0;
          for (int e = 0; e < C * S; ++e) dot[(size_t)p * CS + e] = 0.0;
        }
        if (keep)
        {
          for (int e = 0; e < C * S; ++e) kv[(size_t)p * CS + e] = 0.0;
          ke[p] = 0;
        }
      }
    }
    if (!eval)
    {
      __syncthreads();
      continue;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t_lnl += __shfl_down(t_lnl, off, 64);
    if (lane == 0) sh_ws[0][wid] = t_lnl;
    __syncthreads(); // (also: the products and exponents of every lane are in memory for the probes' lanes)
    if (tid == 0)
    {
      double lkb = 0.0;
      for (int wv = 0; wv < NW; ++wv) lkb += sh_ws[0][wv];
      res.lkBegin[i] = lkb;
      brlen_begin(&st, sh_len[i], lkb, a.tol, q.l_min, q.l_max, a.n_iter_max, a.cap);
      sh_warn = 0; // src/lk.c:669
    }
    __syncthreads();

    // ---- Br_Len_Spline on the products: brlen_opt_kernel's loop
    {
      int stid = tid; // (as jt above)
      asm volatile("" : "+v"(stid));
      DlkIn<S> in[R];
#pragma unroll
      for (int u = 0; u < R; ++u)
        if (stid + u * W < total) triple_fetch<S, CP>(q, k, dot, fact, stid + u * W, in[u]);
      while (!st.done)
      {
        double l = st.l;
        if (l < q.l_min) l = q.l_min; // src/lk.c:673-674: the clamped value is what the search keeps
        else if (l > q.l_max) l = q.l_max;
        dlk_expl_from_len<S>(sh_tab, l, true, C, q.eval_dev, q.rates_dev, q.br_len_mult, q.l_min, q.l_max, stid, W);
        __syncthreads();
        double s_lnl = 0.0, s_dlnl = 0.0;
#pragma unroll
        for (int u = 0; u < R; ++u)
        {
          const int gl = stid + u * W;
          if (gl < total)
          {
            double c0, c1;
            dlk_lane<S, CP>(q, k, sh_tab, &sh_warn, gl, in[u], c0, c1);
            s_lnl += c0;
            s_dlnl += c1;
          }
          __builtin_amdgcn_sched_barrier(0); // (one round's working set at a time)
        }
#pragma unroll 1
        for (int gl = stid + R * W; gl < total; gl += W)
        {
          DlkIn<S> x;
          triple_fetch<S, CP>(q, k, dot, fact, gl, x);
          double c0, c1;
          dlk_lane<S, CP>(q, k, sh_tab, &sh_warn, gl, x, c0, c1);
          s_lnl += c0;
          s_dlnl += c1;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
        {
          s_lnl += __shfl_down(s_lnl, off, 64);
          s_dlnl += __shfl_down(s_dlnl, off, 64);
        }
        if (lane == 0)
        {
          sh_ws[0][wid] = s_lnl;
          sh_ws[1][wid] = s_dlnl;
        }
        __syncthreads();
        if (tid == 0)
        {
          double s0 = 0.0, s1 = 0.0;
          for (int wv = 0; wv < NW; ++wv)
          {
            s0 += sh_ws[0][wv];
            s1 += sh_ws[1][wv];
          }
          st.l = l;
          brlen_step(&st, s0, s1, sh_warn);
          sh_warn = 0; // :669, for the next probe
        }
        __syncthreads();
      }
    }
    if (tid == 0)
    { // src/optimiz.c:2460-2461, then Br_Len_Opt's :632, :654-661
      int status = st.status;
      if (status < 3 && st.best_lnL < res.lkBegin[i] - a.tol) status = kTripleLkEnd;
      sh_len[i]      = st.best_l;
      res.length[i]  = st.best_l;
      res.lnL        = st.best_lnL;
      res.dLnL       = st.c_dlnL;
      res.evaluations[i] = st.evals;
      res.status[i]  = status;
      res.warning    = st.warn;
      sh_stop        = status >= 3;
    }
    __syncthreads();
    if (sh_stop) break;
    build_matrix(i);
    __syncthreads();
  }

  if (tid == 0) a.out[cand] = res;
}

static int triple_run(Instance *I, const phyhip_triple_candidate *cand, int count, int iterMax, double tol, int keep, phyhip_triple_result *out)
{
  static const char *const who = "phyhip_optimise_triples";
  int rc;
  if ((rc = refuse_kind(I, who, kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop | kRefuseStates))) return rc;
  if (I->NE != 1) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d eigen systems", who, I->NE);
  if (I->C < 1 || I->C > kTripleMaxCategories) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d categories", who, I->C);
  if (I->P > kTripleMaxPatterns)
    return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for more than %lld patterns (%lld): run Triple_Dist edge by edge", who,
                kTripleMaxPatterns, I->P);
  if (iterMax < 1 || iterMax > kTripleIterMax) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "iterMax %d (1..%d)", iterMax, kTripleIterMax);
  if (!(tol > 0.0)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "tol %g (must be > 0)", tol);
  for (int k = 0; k < count; ++k)
    for (int i = 0; i < 3; ++i)
    {
      if ((rc = check_partial_index(I, cand[k].partials[i], true))) return fail(rc, "%s: candidate %d: %s", who, k, std::string(g_err).c_str());
      if (cand[k].partials[i] < I->tips && !(cand[k].flags & PHYHIP_TRIPLE_NODE_IS_LEFT(i)))
        return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d: tip %d as the left operand of edge %d", who, k, cand[k].partials[i], i);
      if (std::isnan(cand[k].length[i])) return fail(PHYHIP_ERROR_FLOATING_POINT, "%s: candidate %d: length %d is NaN", who, k, i);
    }
  auto &U = side_of(I).triple;
  U.keep_valid = false;
  for (int k = 0; k < count; ++k)
    for (int i = 0; i < 3; ++i) devirtualise(I, cand[k].partials[i]);
  if ((rc = flush_sync(I))) return rc; // (queued matrix work and partial updates first: the path updates of the caller are seen)
  if ((rc = upload_masks(I))) return rc;

  const TripleLayout size(I->P, I->S, I->C, 0);
  U.lay = TripleLayout(I->P, I->S, I->C, scan_chunk(U.max_bytes, size.fixed, size.per, count));
  const TripleLayout &L = U.lay;
  if ((rc = U.work.reserve(L.total, who))) return rc;
  TripleParams a;
  memset(&a, 0, sizeof a);
  DlkParams &q = a.q;
  q.wght = I->d_wght; q.cat_w = I->d_catw; q.pi = I->d_pi; q.invar = I->d_invar;
  q.P = I->P; q.C = I->C; q.invar_model = I->invar_model; q.apply_scaling = I->apply_scaling; q.with_derivative = 1; q.pinvar = I->pinvar;
  q.eval_dev = I->d_eval; q.rates_dev = I->d_catr; q.br_len_mult = I->br_len_mult; q.l_min = I->l_min; q.l_max = I->l_max;
  a.tip_codes = I->d_tipcodes; a.code_masks = I->d_masks; a.partials = I->d_partials; a.scales = I->d_scales;
  a.U = I->d_evec; a.V = I->d_ivec; a.R = I->d_eval;
  a.Ppad = I->Ppad; a.Pe = (long long)L.exp_ints; a.tips = I->tips;
  a.tol = tol; a.n_iter_max = iterMax; a.cap = brlen_trip_cap(I->l_min, I->l_max);
  a.keep = U.work.at<double>(L.keep); a.mats = U.work.at<double>(L.mats); a.dot = U.work.at<double>(L.dot); a.fact = U.work.at<int>(L.fact);
  phyhip_triple_candidate *d_recs = U.work.at<phyhip_triple_candidate>(L.recs);
  phyhip_triple_result    *d_out = U.work.at<phyhip_triple_result>(L.out);
  a.recs = d_recs; a.out = d_out;

  const int layout = layout_of(I);
  SideTimer tm(I);
  long long evals = 0;
  rc = for_each_chunk(count, L.chunk, keep, [&](size_t first, size_t n, int keep_cand) {
    HIPCHK(hipMemcpyAsync(d_recs, cand + first, n * sizeof *cand, hipMemcpyHostToDevice, I->stream));
    HIPCHK(hipMemsetAsync(d_out, 0xff, n * sizeof *d_out, I->stream)); // (a record nobody wrote reads as status -1 everywhere)
    a.keep_cand = keep_cand;
    const int rt = side_timed(tm, I, U.prof_ms, [&] {
      return dispatch_shape(I, [&](auto s, auto cp) {
        constexpr int S_ = decltype(s)::value, CP_ = decltype(cp)::value;
        if constexpr (CP_ <= 8)
        {
          constexpr int LS = S_ == 4 ? 2 : 1; // the instance's own layout of that state count (phyhip_layout.hpp)
          if (layout == LS) hipLaunchKernelGGL((triple_kernel<S_, CP_, LS>), dim3((unsigned)n), dim3(kTripleThreads<S_>), 0, I->stream, a);
          else if (layout == 0) hipLaunchKernelGGL((triple_kernel<S_, CP_, 0>), dim3((unsigned)n), dim3(kTripleThreads<S_>), 0, I->stream, a);
          else return fail(PHYHIP_ERROR_GENERAL, "%s: buffer layout %d at %d states", who, layout, S_);
        }
        return 0;
      });
    });
    if (rt) return rt;
    HIPCHK(hipMemcpy(out + first, d_out, n * sizeof *d_out, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k)
    {
      const phyhip_triple_result &r = out[first + k];
      if (r.status[0] < 0) return fail(PHYHIP_ERROR_GENERAL, "%s: candidate %zu finished without handing its result over", who, first + k);
      for (int i = 0; i < 3; ++i) evals += r.evaluations[i];
    }
    return 0;
  });
  if (rc) return rc;
  U.keep_valid = keep >= 0 && out[keep].status[2] >= 0 && out[keep].status[2] < 3;
  if (I->prof)
  {
    ++U.prof_n;
    U.prof_evals += evals;
  }
  // the Lk(b) / dLk calls that follow can be served resident again; the flag the host reads (phyhip_get_numerical_warning) is the
  // last candidate's last evaluation's
  side_stream_drained(I);
  *I->h_warn      = out[count - 1].warning;
  I->warn_current = true;
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

int phyhip_optimise_triples(int instance, const phyhip_triple_candidate *candidates, int count, int iterMax, double tol, int keepCandidate,
                            phyhip_triple_result *outResults)
{
  static const char *const who = "phyhip_optimise_triples";
  if (count < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate count %d", who, count);
  if (count > 0 && (!candidates || !outResults)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: a NULL array for %d candidates", who, count);
  if (keepCandidate < -1 || keepCandidate >= count) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: keepCandidate %d of %d candidates", who, keepCandidate, count);
  if (get_group(instance))
    return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for one-process sharded instances (each probe needs every shard's sums)", who);
  GET_INST(I, instance);
  if (count == 0) return PHYHIP_SUCCESS;
  return triple_run(I, candidates, count, iterMax, tol, keepCandidate, outResults);
}

int phyhip_get_triple_partials(int instance, int which, double *outPartials, int *outScaleFactors)
{
  static const char *const who = "phyhip_get_triple_partials";
  if (which < 0 || which > 2) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: which %d (0..2)", who, which);
  if (get_group(instance)) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for one-process sharded instances", who);
  GET_INST(I, instance);
  auto &U = side_of(I).triple;
  if (!U.keep_valid || !U.work.ptr)
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no phyhip_optimise_triples call before it that kept a candidate which ran to its end", who);
  if (outPartials) HIPCHK(hipMemcpy(outPartials, U.work.at<double>(U.lay.keep_of(which)), U.lay.vec_bytes, hipMemcpyDeviceToHost));
  if (outScaleFactors) HIPCHK(hipMemcpy(outScaleFactors, U.work.at<int>(U.lay.exps_of(which)), (size_t)I->P * sizeof(int), hipMemcpyDeviceToHost));
  return PHYHIP_SUCCESS;
}

int phyhip_set_triple_work_space(int instance, long long maxBytes)
{
  if (maxBytes < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_set_triple_work_space: %lld bytes", maxBytes);
  if (get_group(instance)) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "phyhip_set_triple_work_space: not built for one-process sharded instances");
  GET_INST(I, instance);
  side_of(I).triple.max_bytes = maxBytes ? (size_t)maxBytes : kRegraftWorkBytes;
  return PHYHIP_SUCCESS;
}

int phyhip_profile_read_triples(int instance, double *outKernelMs, int *outCalls, long long *outEvaluations)
{
  double    ms = 0.0;
  int       n = 0;
  long long ev = 0;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).triple;
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
