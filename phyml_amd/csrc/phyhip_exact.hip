// phyhip_exact.hip -- the per-pattern outputs of Lk_Core as the REFERENCE's doubles: phyhip_calculate_edge_site_outputs_exact
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// The evaluation kernels of the hot path take the general product for every pattern and the device library's log(): their lnL is
// the reference's to ~1e-13, their per-site arrays to 1e-10 / 1e-12 -- not to the bit.  Host readers of those arrays (aLRT /
// SH-like supports, --print_site_lnl, cv.c, ancestral reconstruction) compare and rank them, so a binding that wants the CPU
// run's supports asks HERE: one kernel of its own beside the hot path, one lane per pattern, that walks Lk_Core's operations in
// Lk_Core's order (src/lk.c:767-861 with src/avx.c:110-215 and Pull_Scaling_Factors; the tests hold it to the CPU restatement
// under oracle/, arith = 1) --
//   * right side an unambiguous tip (one allowed state s): pi[s] * norm(P[s][.] o left), products rounded one by one;
//   * otherwise acc[k] = fused chain over the left states from 0, acc[k] * (rght[k] * pi[k]), blockwise (q0+q2)+(q1+q3);
//   * the category sum with rounded products, the +I mix and the final subtraction fused where the reference's binary fuses them
//     (site * (1 - pinvar) + inv * pinvar as fma(site, 1 - pinvar, inv * pinvar); log(site) - LOG2 * fact as fma(-fact, LOG2, log)),
//   * log and exp the reference's libm's (phyhip_log.hpp, phyhip_exp.hpp).
// It writes buffers of its own: what the evaluation kernels left (site outputs, warning flag, results) stays as it was.
#include "phyhip_side.hpp"
#include "phyhip_layout.hpp"
#include "phyhip_log.hpp"

namespace phyhip_host
{

struct ExactParams
{
  const uint8_t  *tip_codes;  // tip t at t * Ppad (4 states: the byte is the state set; 20: an index into code_masks)
  const uint32_t *code_masks;
  const double   *wght, *pi, *cat_w;
  const short    *invar;
  double         *site_lnl, *site_lk, *site_cat; // [P], [P], [P][C]
  int            *fact, *warn;                   // [P], [1]
  long long       P, Ppad;
  int             C, tips, layout; // layout: 0 [pattern][category][state], 1 fragment-major (aa_off), 2 pattern-minor state pairs
  int             parent, child, apply_scaling, invar_model;
  double          pinvar;
};

// (phyhip_layout.hpp)
template <int S> __device__ __forceinline__ size_t exact_off(const ExactParams &q, int b, long long p, int c, int s)
{
  return partial_off<S>(q.layout, q.P, q.Ppad, q.C, b, p, c, s);
}

template <int S> __device__ __forceinline__ uint32_t exact_tip_mask(const ExactParams &q, int tip, long long p)
{
  return tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, tip, p);
}

// One lane per pattern.  20 states: the category's matrix (400 doubles) is staged in LDS by the workgroup, category after
// category (every lane of the workgroup takes part in the barriers, also those without a pattern or without weight).
template <int S>
__global__ __launch_bounds__(256) void exact_site_kernel(const ExactParams q, const double *__restrict__ pm,
                                                         const double *__restrict__ partials, const int *__restrict__ scales)
{
  __shared__ double Ms[S == 20 ? 400 : 2];
  const long long   p = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool        in = p < q.P;
  const bool        act = in && q.wght[p] > kSmall;              // src/lk.c:632
  const bool        ltip = q.parent < q.tips, rtip = q.child < q.tips; // (the same for the whole grid)
  const int         lb = q.parent - q.tips, rb = q.child - q.tips;
  double            x[S], y[S];
  bool              onehot = false; // only a right-hand tip can be "observed" (src/lk.c:610-621)
  int               state = 0;
  if (act && ltip)
  {
    const uint32_t m = exact_tip_mask<S>(q, q.parent, p);
#pragma unroll
    for (int j = 0; j < S; ++j) x[j] = ((m >> j) & 1u) ? 1.0 : 0.0;
  }
  if (act && rtip)
  {
    const uint32_t m = exact_tip_mask<S>(q, q.child, p);
#pragma unroll
    for (int j = 0; j < S; ++j) y[j] = ((m >> j) & 1u) ? 1.0 : 0.0;
    onehot = __popc(m) == 1;
    state  = onehot ? __ffs((int)m) - 1 : 0;
  }

  double site = 0.0;
  for (int c = 0; c < q.C; ++c)
  {
    const double *__restrict__ Mg = pm + (size_t)c * S * S; // rows: right-side state
    if (S == 20)
    {
      __syncthreads();
      for (int i = threadIdx.x; i < S * S; i += 256) Ms[i] = Mg[i];
      __syncthreads();
    }
    if (!act) continue;
    if (!ltip)
    {
#pragma unroll
      for (int j = 0; j < S; ++j) x[j] = partials[exact_off<S>(q, lb, p, c, j)];
    }
    double lkc;
    if (onehot)
    { // src/avx.c:117-123, 157-176: elementwise products, per-lane sums in block order, the horizontal norm, then pi[s]
      double lane[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int b4 = 0; b4 < S / 4; ++b4)
      {
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
          const int    l = b4 * 4 + k;
          const double prod = (S == 20 ? Ms[state * S + l] : Mg[state * S + l]) * x[l];
          lane[k] = (S == 4) ? prod : lane[k] + prod;
        }
      }
      lkc = q.pi[state] * ((lane[0] + lane[2]) + (lane[1] + lane[3]));
    }
    else
    { // src/avx.c:130-148, 184-210
      if (!rtip)
      {
#pragma unroll
        for (int j = 0; j < S; ++j) y[j] = partials[exact_off<S>(q, rb, p, c, j)];
      }
      lkc = 0.0;
#pragma unroll
      for (int b4 = 0; b4 < S / 4; ++b4)
      {
        double t[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
        {
          const int k = b4 * 4 + kk;
          double    a = 0.0;
#pragma unroll
          for (int i = 0; i < S; ++i) a = __builtin_fma(S == 20 ? Ms[k * S + i] : Mg[k * S + i], x[i], a);
          t[kk] = a * (y[k] * q.pi[k]);
        }
        const double nrm = (t[0] + t[2]) + (t[1] + t[3]);
        lkc = (S == 4) ? nrm : lkc + nrm;
      }
    }
    q.site_cat[(size_t)p * q.C + c] = lkc; // Pull_Scaling_Factors' copy, src/lk.c:2801
    const double t = lkc * q.cat_w[c];     // src/lk.c:818
    site = site + t;
  }

  if (!in) return;
  if (!act)
  { // the reference leaves such a pattern's entries as they were; here they are zero
    for (int c = 0; c < q.C; ++c) q.site_cat[(size_t)p * q.C + c] = 0.0;
    q.site_lnl[p] = 0.0; q.site_lk[p] = 0.0; q.fact[p] = 0;
    return;
  }
  // Pull_Scaling_Factors, SCALE_FAST: src/lk.c:2701-2705, 2777-2801
  int f = 0;
  if (q.apply_scaling) f = (ltip ? 0 : scales[(size_t)lb * q.Ppad + p]) + (rtip ? 0 : scales[(size_t)rb * q.Ppad + p]);
  // src/lk.c:820-856 as the reference's binary has it: the +I mix one fused operation, the reference's log / exp with the LOG2 term
  // fused, every output present (tests/test_gpu_exact_site.py holds them to the reference's bits).  Patterns without weight have
  // returned above: the weight test passes by construction and the weighted term is not used.
  double term;
  site_tail<TailMix::fused, TailLibm::reference>(term, q, (size_t)p, 1.0, site, f, PlainStore());
}

// One plain instance: its patterns into the caller's arrays (any may be NULL; wght_out receives its pattern weights)
static int exact_run(Instance *I, int parent, int child, int pm, double *lnl, double *lk, double *cat, int *fact, double *wght_out,
                     int *warn_out)
{
  static const char *const who = "phyhip_calculate_edge_site_outputs_exact";
  int rc;
  if ((rc = refuse_kind(I, who, kRefuseClassAxis | kRefuseGenericLoop))) return rc;
  if ((rc = check_partial_index(I, parent, true))) return rc;
  if ((rc = check_partial_index(I, child, true))) return rc;
  if (pm < 0 || pm >= I->nmat) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "matrix index %d", pm);
  if (I->C < 1 || I->C > kMaxCategories) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d categories", who, I->C);
  if ((rc = refuse_kind(I, who, kRefuseStates))) return rc;
  devirtualise(I, parent); devirtualise(I, child);
  if ((rc = flush_sync(I))) return rc;
  if ((rc = upload_masks(I))) return rc;
  const size_t P = (size_t)I->P, nd = P * (size_t)(2 + I->C);
  WorkSpace &out = side_of(I).exact.out;
  if ((rc = out.reserve(nd * sizeof(double) + (P + 1) * sizeof(int), who))) return rc;
  ExactParams q;
  memset(&q, 0, sizeof q);
  q.tip_codes = I->d_tipcodes; q.code_masks = I->d_masks; q.wght = I->d_wght; q.pi = I->d_pi; q.cat_w = I->d_catw; q.invar = I->d_invar;
  q.site_lnl = (double *)out.ptr; q.site_lk = q.site_lnl + P; q.site_cat = q.site_lk + P;
  q.fact = (int *)(q.site_cat + P * (size_t)I->C); q.warn = q.fact + P;
  q.P = I->P; q.Ppad = I->Ppad; q.C = I->C; q.tips = I->tips; q.layout = layout_of(I);
  q.parent = parent; q.child = child; q.apply_scaling = I->apply_scaling; q.invar_model = I->invar_model; q.pinvar = I->pinvar;
  HIPCHK(hipMemsetAsync(q.warn, 0, sizeof(int), I->stream));
  const double *pmat = I->d_pmats + (size_t)pm * I->C * I->S * I->S;
  const dim3    grid((unsigned)((I->P + 255) / 256)), block(256);
  if (I->S == 4)
    hipLaunchKernelGGL(exact_site_kernel<4>, grid, block, 0, I->stream, q, pmat, (const double *)I->d_partials, (const int *)I->d_scales);
  else
    hipLaunchKernelGGL(exact_site_kernel<20>, grid, block, 0, I->stream, q, pmat, (const double *)I->d_partials, (const int *)I->d_scales);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(I->stream));
  if (lnl) HIPCHK(hipMemcpy(lnl, q.site_lnl, P * sizeof(double), hipMemcpyDeviceToHost));
  if (lk) HIPCHK(hipMemcpy(lk, q.site_lk, P * sizeof(double), hipMemcpyDeviceToHost));
  if (cat) HIPCHK(hipMemcpy(cat, q.site_cat, P * (size_t)I->C * sizeof(double), hipMemcpyDeviceToHost));
  if (fact) HIPCHK(hipMemcpy(fact, q.fact, P * sizeof(int), hipMemcpyDeviceToHost));
  if (wght_out) HIPCHK(hipMemcpy(wght_out, I->d_wght, P * sizeof(double), hipMemcpyDeviceToHost));
  int w = 0;
  HIPCHK(hipMemcpy(&w, q.warn, sizeof(int), hipMemcpyDeviceToHost));
  if (w) *warn_out = 1;
  return PHYHIP_SUCCESS;
}

// the ordered sum of Lk_Core over the downloaded arrays: src/lk.c:856, patterns in ascending order, products rounded
static double exact_sum(const double *w, const double *lnl, long long P)
{
  double sum = 0.0;
  for (long long p = 0; p < P; ++p)
    if (w[p] > kSmall)
    {
      const volatile double t = w[p] * lnl[p];
      sum = sum + t;
    }
  return sum;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

int phyhip_calculate_edge_site_outputs_exact(int instance, int parentBufferIndex, int childBufferIndex, int probabilityIndex,
                                             double *c_lnL_sorted, double *cur_site_lk, double *unscaled_site_lk_cat,
                                             int *fact_sum_scale, double *outSumLogLikelihood, int *outNumericalWarning)
{
  std::vector<double> own_lnl, wght;
  double             *lnl = c_lnL_sorted, *w = nullptr;
  int                 warn = 0;
  // (the sum is formed on the host from the downloaded array -- a sharded group: over the concatenated one, so that sharding
  // does not change it)
  auto host_arrays = [&](long long P) {
    if (!outSumLogLikelihood) return;
    wght.resize((size_t)P);
    w = wght.data();
    if (!lnl) { own_lnl.resize((size_t)P); lnl = own_lnl.data(); }
  };
  long long P = 0;
  const Group *const G = get_group_nodrain(instance); // (for the size of the whole only, taken when the first shard is entered)
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long) {
    if (lo == 0) host_arrays(P = G ? G->P : I->P);
    return exact_run(I, parentBufferIndex, childBufferIndex, probabilityIndex, lnl ? lnl + lo : nullptr, cur_site_lk ? cur_site_lk + lo : nullptr,
                     unscaled_site_lk_cat ? unscaled_site_lk_cat + lo * I->C : nullptr, fact_sum_scale ? fact_sum_scale + lo : nullptr,
                     w ? w + lo : nullptr, &warn);
  });
  if (rc < 0) return rc;
  if (outSumLogLikelihood) *outSumLogLikelihood = exact_sum(w, lnl, P);
  if (outNumericalWarning) *outNumericalWarning = warn;
  return PHYHIP_SUCCESS;
}

} // extern "C"
