// phyhip_regraft.hip -- the regraft scan of an SPR move: K candidates in, K log-likelihoods out, one call:
// phyhip_calculate_regraft_log_likelihoods (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// Test_One_Spr_Target (src/spr.c:590-760) rebuilds, for every target edge of a pruned subtree, the matrices of the two halves of the
// target edge and of b_arrow, runs Update_Partial_Lk(b_arrow, n_link) and evaluates Lk(b_arrow).  After Prune_Subtree the candidates
// are independent of each other: each joins three vectors that exist already -- the two sides of the target edge and the pruned
// subtree.  Here a candidate is a record {child 1, child 2, subtree, three lengths} and the whole list is served by
//   regraft_pmat_kernel<S>   one workgroup per (distinct length of the chunk, category): PMat_Empirical as pmat_kernel has it
//                            (src/models.c:257-326 behind src/lk.c:2280-2316), into the unit's work space -- the instance's matrix
//                            table is neither read nor written;
//   regraft_scan_kernel<S,L> grid (pattern tiles of 256, candidate), one lane per pattern: the vector AVX_Update_Partial_Lk would
//                            store (src/avx.c:380-520: Exex / Exin / Inin are the same fused chains over 0/1 tip vectors, the
//                            all-ones shortcut, the sum of the children's exponents, the 2^256 rule), held in registers (4 states)
//                            or computed a second time once the scaling decision is known (20 states: pass 1 finds the largest
//                            C*S value, pass 2 evaluates), then Lk_Core's product with the subtree through the third matrix and
//                            the shared site tail (phyhip_tail.hpp: fused +I mix, the ported log).  The vector goes to memory only
//                            for the one candidate the caller asked to keep.  No scratch, no atomics;
//   regraft_sum_kernel       one thread per candidate adds its tile sums in ascending tile order.
// The sum of a candidate is formed in one fixed order -- lane, the wave's shuffle tree, the waves in wave order, the tiles in
// ascending order -- so its bits depend on the candidate alone: not on K, its position, or how the call was cut into chunks.
// Consecutive records that name the same subtree do NOT share it in registers: a workgroup serves one candidate, and the subtree's
// 256-pattern tile is re-read by the next candidate's workgroup (from L2 where the list is short enough to keep it there).
// The lnL takes the general product at every pattern (no observed-tip special case), like the launched evaluation kernels: it is
// the reference's to ~1e-13, the KEPT vector and the matrices are the reference's doubles (tests/test_gpu_regraft.py).
// It writes a work space of its own: partials, scale vectors, the matrix table, site outputs, dot_prod and the warning flag of the
// instance stay as they were.
// Below it the same scan for a mixture: phyhip_calculate_mixture_regraft_log_likelihoods takes the class instances, and one kernel
// loops over the classes and combines them as MIXT_Lk does (mixregraft_matrices_kernel, mixregraft_classes_kernel; their header
// stands in front of them).  Operand fetch, joined vector, product and the matrix body are device functions both scans call
// (phyhip_regraft_dev.hpp, which phyhip_triple.hip includes too).
// Host side: each scan brings its refusals, its kernel parameters and its kernels; the candidate checks, the reservation and the chunk
// loop are phyhip_scan.hpp's, every offset and the chunk size phyhip_scan_plan.hpp's (ScanLayout, left on the unit for the getters).
#include <memory>

#include "phyhip_regraft_dev.hpp" // the matrix body, operand fetch, joined vector and product: shared with phyhip_triple.hip
#include "phyhip_scan.hpp"        // the host driver: candidate checks, work-space reservation, the chunk loop

namespace phyhip_host
{

constexpr int kRegraftMaxCategories = 8; // the 4-state kernel holds C * S values in registers

struct RegraftPmatParams
{
  const double *lengths; // [slot] raw edge lengths
  const double *U, *V, *R, *rates;
  double       *mats;    // [slot][C][S][S]
  double        br_len_mult, l_min, l_max;
  int          *flags;   // [n_flags] the launch's warning flags: zeroed here, in front of the scan kernel
  int           C, n_flags;
};

struct RegraftParams
{
  const uint8_t    *tip_codes;
  const uint32_t   *code_masks;
  const double     *wght, *pi, *cat_w;
  const short      *invar;     // NULL without +I
  const double     *partials;
  const int        *scales;
  const RegraftRec *recs;      // [candidate of the launch]
  const double     *mats;      // [slot][C][S][S]
  double           *tile_sums; // [candidate][tiles]; behind the launch's tile sums its warning flags, [candidate] ints
  double           *keep;      // [P][C][S], host order: the kept candidate's vector; behind it its exponents, [P] ints
  int               keep_cand; // candidate of the launch whose vector is kept, or -1
  long long         P, Ppad;
  int               C, tips, apply_scaling; // (+I: invar is not NULL; the tiles of a candidate: gridDim.x)
  double            pinvar;
};

template <int S> __global__ __launch_bounds__(256) void regraft_pmat_kernel(const RegraftPmatParams q)
{
  __shared__ double expt[S], tmp[S * S], rsum[S];
  const int m = blockIdx.x, c = blockIdx.y;
  if (m == 0 && c == 0)
    for (int k = threadIdx.x; k < q.n_flags; k += 256) q.flags[k] = 0;
  regraft_pmat_body<S>(q.lengths[m], q.U, q.V, q.R, q.rates[c], q.br_len_mult, q.l_min, q.l_max, q.mats + ((size_t)m * q.C + c) * S * S, expt, tmp,
                       rsum);
}

// One lane per pattern, one candidate per blockIdx.y (which operands are tips is the same for the whole workgroup).  4 states: the
// candidate's 3 C matrices are staged in LDS once (3 KB; read at wave-uniform addresses: scalar loads of 96 doubles per category
// spilled scalar registers) and the C*S values wait in registers for the scaling decision.  20 states: the
// matrices of one category are staged in LDS by the workgroup (two in the first pass, three in the second) -- every lane of the
// workgroup takes part in the barriers, also those without a pattern or without weight.  L: the layout of the instance's buffers
// (phyhip_layout.hpp: 0 host order, 1 fragment-major 20-state, 2 pattern-minor 4-state pairs) at compile time -- as a run-time
// value its three address forms cost the 20-state kernel scalar registers it does not have.
template <int S, int L> __global__ __launch_bounds__(256) void regraft_scan_kernel(const RegraftParams q)
{
  constexpr int SS = S * S;
  __shared__ double Ms[S == 20 ? 3 * SS : 3 * kRegraftMaxCategories * SS]; // 20: one category's three; 4: [which][category]
  __shared__ double wsum[4], pis[S]; // (pi as 2 S scalar registers next to the kernel's arguments spilled scalar registers at 20 states)
  if (threadIdx.x < S) pis[threadIdx.x] = q.pi[threadIdx.x]; // (read behind the barriers of the matrix staging)
  const RegraftRec r = q.recs[blockIdx.y];
  const long long  p = (long long)blockIdx.x * kRegraftTile + threadIdx.x;
  const bool       in = p < q.P;
  const double     w = in ? q.wght[p] : 0.0;
  const bool       act = in && w > kSmall; // src/avx.c:399, src/lk.c:632
  const bool       keep = q.keep_cand == (int)blockIdx.y;
  const bool       sub_left = (r.flags & PHYHIP_REGRAFT_SUBTREE_IS_LEFT) != 0;
  // (the three matrices as 32-bit offsets, the exponents of the kept vector behind it: the 20-state kernel has no scalar registers to spare)
  const double *__restrict__ G = q.mats;
  const unsigned g1 = (unsigned)r.m1 * (unsigned)(q.C * SS), g2 = (unsigned)r.m2 * (unsigned)(q.C * SS), g3 = (unsigned)r.m3 * (unsigned)(q.C * SS);

  uint32_t k1 = 0, k2 = 0, k3 = 0;
  int      sc = 0, s3 = 0;
  if (act)
  {
    if (r.c1 < q.tips) k1 = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, r.c1, p);
    else sc += q.scales[(size_t)(r.c1 - q.tips) * q.Ppad + p];
    if (r.c2 < q.tips) k2 = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, r.c2, p);
    else sc += q.scales[(size_t)(r.c2 - q.tips) * q.Ppad + p]; // src/avx.c:462-464
    if (r.sub < q.tips) k3 = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, r.sub, p);
    else s3 = q.scales[(size_t)(r.sub - q.tips) * q.Ppad + p];
  }

  // ---- pass 1: the largest of the C*S values (src/avx.c:497-502; `>`: a NaN never becomes the maximum) ----------------------------
  double oc[S == 4 ? kRegraftMaxCategories * S : 1];
  double mx = -__builtin_huge_val();
  if (S == 4)
  {
    for (int i = threadIdx.x; i < q.C * SS; i += 256)
    {
      Ms[i]                                  = G[g1 + i];
      Ms[kRegraftMaxCategories * SS + i]     = G[g2 + i];
      Ms[2 * kRegraftMaxCategories * SS + i] = G[g3 + i];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kRegraftMaxCategories; ++c)
      if (c < q.C && act)
      {
        double o[S];
        regraft_join<S, L>(q, r, k1, k2, p, c, Ms + c * SS, Ms + (kRegraftMaxCategories + c) * SS, o);
#pragma unroll
        for (int i = 0; i < S; ++i)
        {
          if constexpr (S == 4) oc[c * S + i] = o[i];
          mx = (o[i] > mx) ? o[i] : mx;
        }
      }
  }
  else
  {
    for (int c = 0; c < q.C; ++c)
    {
      __syncthreads();
      for (int i = threadIdx.x; i < SS; i += 256)
      {
        Ms[i]      = G[g1 + c * SS + i];
        Ms[SS + i] = G[g2 + c * SS + i];
      }
      __syncthreads();
      if (!act) continue;
      double o[S];
      regraft_join<S, L>(q, r, k1, k2, p, c, Ms, Ms + SS, o);
#pragma unroll
      for (int i = 0; i < S; ++i) mx = (o[i] > mx) ? o[i] : mx;
    }
  }
  const bool scale = act && mx < kInvTwoToLarge && q.apply_scaling; // src/avx.c:504-510
  if (scale) sc += kLarge;

  // ---- pass 2: the vector as stored, and Lk_Core's product with the subtree (src/avx.c:130-148, 184-210) ---------------------------
  double site = 0.0;
  double y[S];
  if (act && r.sub < q.tips) regraft_operand<S, L>(q, r.sub, k3, p, 0, y);
  auto category = [&](const int c) {
    if (S == 20)
    {
      __syncthreads();
      for (int i = threadIdx.x; i < SS; i += 256)
      {
        Ms[i]          = G[g1 + c * SS + i];
        Ms[SS + i]     = G[g2 + c * SS + i];
        Ms[2 * SS + i] = G[g3 + c * SS + i];
      }
      __syncthreads();
    }
    if (!act) return;
    double o[S];
    if constexpr (S == 4)
    {
#pragma unroll
      for (int i = 0; i < S; ++i) o[i] = oc[c * S + i];
    }
    else
      regraft_join<S, L>(q, r, k1, k2, p, c, Ms, Ms + SS, o);
    if (scale)
    { // multiplication by 2^256 is exact
#pragma unroll
      for (int i = 0; i < S; ++i) o[i] *= kTwoToLarge;
    }
    if (keep)
    {
      double *__restrict__ dst = q.keep + ((size_t)p * q.C + c) * S;
#pragma unroll
      for (int i = 0; i < S; ++i) dst[i] = o[i];
    }
    if (r.sub >= q.tips) regraft_operand<S, L>(q, r.sub, k3, p, c, y);
    const double *__restrict__ M3 = Ms + (S == 20 ? 2 * SS : (2 * kRegraftMaxCategories + c) * SS); // rows: the right-side state
    const double lkc = regraft_product<S>(M3, o, y, pis, sub_left);
    const double t = lkc * q.cat_w[c]; // src/lk.c:818
    site = site + t;
  };
  if constexpr (S == 4)
  { // (unrolled: the registers of pass 1 are named at compile time)
#pragma unroll
    for (int c = 0; c < kRegraftMaxCategories; ++c)
      if (c < q.C) category(c);
  }
  else
    for (int c = 0; c < q.C; ++c) category(c);

  double contrib = 0.0;
  if (act)
  {
    if (keep) reinterpret_cast<int *>(q.keep + (size_t)q.P * q.C * S)[p] = sc; // (its exponents lie behind it)
    RegraftTailQ tq;
    tq.invar = q.invar; tq.pi = q.pi; tq.site_lnl = nullptr; tq.site_lk = nullptr; tq.fact = nullptr; tq.warn = reinterpret_cast<int *>(q.tile_sums + (size_t)gridDim.y * gridDim.x) + blockIdx.y;
    tq.invar_model = q.invar != nullptr; tq.apply_scaling = q.apply_scaling; tq.pinvar = q.pinvar;
    const int f = q.apply_scaling ? sc + s3 : 0; // Pull_Scaling_Factors, SCALE_FAST: src/lk.c:2701-2705, 2777-2801
    site_tail<TailMix::fused, TailLibm::reference>(contrib, tq, (size_t)p, w, site, f, NoStore());
  }
  else if (in && keep)
  { // the reference leaves such a pattern's entries as they were; here they are zero
    for (int e = 0; e < q.C * S; ++e) q.keep[(size_t)p * q.C * S + e] = 0.0;
    reinterpret_cast<int *>(q.keep + (size_t)q.P * q.C * S)[p] = 0;
  }

  // the wave's fixed shuffle tree, then the waves in wave order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) contrib += __shfl_down(contrib, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) q.tile_sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void regraft_sum_kernel(const double *__restrict__ tile_sums, double *__restrict__ out, const int tiles, const int n)
{
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  double sum = 0.0;
  for (int t = 0; t < tiles; ++t) sum += tile_sums[(size_t)k * tiles + t];
  out[k] = sum;
}

// ---- the scan of a mixture: the same K candidates over every class tree, combined as MIXT_Lk combines them -------------------------
// A class is an instance of one category with its own eigen system, frequencies, rate and tip data; the class trees share topology
// and buffer numbering, so one record serves all of them.  Per candidate and class the three matrices are built by
//   mixregraft_matrices_kernel<S>   grid (distinct lengths of the chunk, classes): regraft_pmat_body with the class's own eigen system,
//                                   rate, multiplier and clamp, read from the per-class table in the work space;
//   mixregraft_classes_kernel<S,L>  grid (pattern tiles of 256, candidate), one lane per pattern, the classes in a loop inside the
//                                   workgroup: the class's three matrices staged in LDS (3 S S doubles), its joined vector -- S values,
//                                   one category -- in registers at both state counts, so the 2^256 decision needs no second pass;
//                                   x_k = Lk_Core's product, f_k = the sum of the two sides' exponents; then the site loop of MIXT_Lk
//                                   (src/mixt.c:1027-1142) in the operation order of mixture_combine_kernel, accumulated in registers:
//                                   nothing per class and pattern goes to memory except the kept candidate's vectors.
// regraft_sum_kernel adds the tile sums.  The per-class table {buffers, tip data, frequencies, eigen system, rate, clamp, the three
// coefficients} is 128 bytes a class -- 8 KB at 64 classes, more than the kernel-argument segment holds -- and goes up with the records.
struct MixRegraftClass
{
  const uint8_t  *tip_codes;
  const uint32_t *code_masks;
  const double   *partials;
  const int      *scales;
  const double   *pi, *U, *V, *R;
  double          rate, br_len_mult, l_min, l_max;
  double          proba, r_w, e_w;
  int             apply_scaling, pad;
};
static_assert(sizeof(MixRegraftClass) == 128, "the per-class table's entry");

// what the combination needs beside the classes: in the work space in front of the per-class table, not among the kernel's arguments
// (the 20-state kernel has no scalar registers to hold them through the class loop)
struct MixRegraftHead
{
  double       r_sum, e_sum, sum_probas, pinvar;
  const short *invar;      // the +I share of phyhip_set_mixture_invariant_sites on the first instance, or NULL
  double       pi_inv[20]; // frequencies of the invariant class
};
static_assert(sizeof(MixRegraftHead) == 200, "the head in front of the per-class table");
static_assert(sizeof(MixRegraftHead) == kMixRegraftHeadBytes && sizeof(MixRegraftClass) == kMixRegraftClassBytes, "as phyhip_scan_plan.hpp places them");

struct MixRegraftPmatParams
{
  const double          *lengths; // [slot] raw edge lengths of the mixture tree
  const MixRegraftClass *cls;     // [class]
  double                *mats;    // [slot][class][S][S]
  int                   *flags;   // [n_flags] the launch's warning flags: zeroed here
  int                    n_cls, n_flags;
};

struct MixRegraftParams
{
  const MixRegraftClass *cls;       // [class]
  const MixRegraftHead  *head;
  const double          *wght;      // the FIRST instance's pattern weights
  const RegraftRec      *recs;      // [candidate of the launch]
  const double          *mats;      // [slot][class][S][S]
  double                *tile_sums; // [candidate][tiles]; behind the launch's tile sums its warning flags, [candidate] ints
  double                *keep;      // [class][P][S], host order: the kept candidate's vectors; behind them their exponents, [class][P rounded up to even] ints
  long long              P, Ppad;
  int                    n_cls, tips, keep_cand;
};

template <int S> __global__ __launch_bounds__(256) void mixregraft_matrices_kernel(const MixRegraftPmatParams q)
{
  __shared__ double expt[S], tmp[S * S], rsum[S];
  const int m = blockIdx.x, k = blockIdx.y;
  if (m == 0 && k == 0)
    for (int i = threadIdx.x; i < q.n_flags; i += 256) q.flags[i] = 0;
  const MixRegraftClass &c = q.cls[k];
  regraft_pmat_body<S>(q.lengths[m], c.U, c.V, c.R, c.rate, c.br_len_mult, c.l_min, c.l_max, q.mats + ((size_t)m * q.n_cls + k) * S * S, expt, tmp,
                       rsum);
}

template <int S, int L> __global__ __launch_bounds__(256) void mixregraft_classes_kernel(const MixRegraftParams q)
{
  constexpr int SS = S * S;
  __shared__ double Ms[3 * SS], wsum[4], pis[S];
  RegraftRec r;
  if constexpr (S == 20)
  { // read as lane values (a volatile load is no scalar load): as scalars, the address arithmetic of three operands -- 64-bit, hoisted
    // out of the class loop -- takes more scalar registers than the 20-state kernel has, and they spill
    const volatile int *rp = reinterpret_cast<const volatile int *>(q.recs + blockIdx.y);
    r.c1 = rp[0]; r.c2 = rp[1]; r.sub = rp[2]; r.flags = rp[3]; r.m1 = rp[4]; r.m2 = rp[5]; r.m3 = rp[6]; r.pad = 0;
  }
  else
    r = q.recs[blockIdx.y];
  const long long p = (long long)blockIdx.x * kRegraftTile + threadIdx.x;
  const bool      in = p < q.P;
  const double    w = in ? q.wght[p] : 0.0;
  const bool      act = in && w > kSmall; // src/mixt.c:998-1003: a pattern without weight is never evaluated
  const bool       keep = q.keep_cand == (int)blockIdx.y;
  const bool       sub_left = (r.flags & PHYHIP_REGRAFT_SUBTREE_IS_LEFT) != 0;
  int *const       warn = reinterpret_cast<int *>(q.tile_sums + (size_t)gridDim.y * gridDim.x) + blockIdx.y;
  const size_t     MS = (size_t)q.n_cls * SS;
  const size_t     g1 = (size_t)r.m1 * MS, g2 = (size_t)r.m2 * MS, g3 = (size_t)r.m3 * MS;

  double site_lk = 0.0;
#pragma nounroll
  for (int k = 0; k < q.n_cls; ++k)
  {
    const MixRegraftClass &c = q.cls[k];
    __syncthreads(); // (the lanes of the class before have read its matrices)
    for (int i = threadIdx.x; i < SS; i += 256)
    {
      Ms[i]          = q.mats[g1 + k * SS + i];
      Ms[SS + i]     = q.mats[g2 + k * SS + i];
      Ms[2 * SS + i] = q.mats[g3 + k * SS + i];
    }
    if (threadIdx.x < S) pis[threadIdx.x] = c.pi[threadIdx.x];
    __syncthreads();
    double *const kv = q.keep + (size_t)k * q.P * S;
    int *const    ke = reinterpret_cast<int *>(q.keep + (size_t)q.n_cls * q.P * S) + (size_t)k * (((size_t)q.P + 1) & ~(size_t)1);
    if (!act)
    { // the reference leaves such a pattern's entries as they were; here they are zero
      if (in && keep)
      {
        for (int e = 0; e < S; ++e) kv[(size_t)p * S + e] = 0.0;
        ke[p] = 0;
      }
      continue;
    }
    const MixRegraftSrc src{c.partials, q.P, q.Ppad, 1, q.tips};
    uint32_t k1 = 0, k2 = 0, k3 = 0;
    int      sc = 0, s3 = 0;
    if (r.c1 < q.tips) k1 = tip_state_mask<S>(c.tip_codes, c.code_masks, q.Ppad, r.c1, p);
    else sc += c.scales[(size_t)(r.c1 - q.tips) * q.Ppad + p];
    if (r.c2 < q.tips) k2 = tip_state_mask<S>(c.tip_codes, c.code_masks, q.Ppad, r.c2, p);
    else sc += c.scales[(size_t)(r.c2 - q.tips) * q.Ppad + p]; // src/avx.c:462-464
    if (r.sub < q.tips) k3 = tip_state_mask<S>(c.tip_codes, c.code_masks, q.Ppad, r.sub, p);
    else s3 = c.scales[(size_t)(r.sub - q.tips) * q.Ppad + p];

    // the class's joined vector, as AVX_Update_Partial_Lk would store it: one pass, the S values wait in registers for the decision
    double o[S];
    regraft_join<S, L>(src, r, k1, k2, p, 0, Ms, Ms + SS, o);
    double mx = -__builtin_huge_val(); // (src/avx.c:497-502; `>`: a NaN never becomes the maximum)
#pragma unroll
    for (int i = 0; i < S; ++i) mx = (o[i] > mx) ? o[i] : mx;
    if (mx < kInvTwoToLarge && c.apply_scaling)
    { // src/avx.c:504-510; multiplication by 2^256 is exact
#pragma unroll
      for (int i = 0; i < S; ++i) o[i] *= kTwoToLarge;
      sc += kLarge;
    }
    if (keep)
    {
#pragma unroll
      for (int i = 0; i < S; ++i) kv[(size_t)p * S + i] = o[i];
      ke[p] = sc;
    }
    double y[S];
    regraft_operand<S, L>(src, r.sub, k3, p, 0, y);
    // the site loop of MIXT_Lk, as mixture_combine_kernel has it (src/mixt.c:1027-1053).  (The exponent's cap with its store stands in
    // front of the product: behind it the compiler moves the product's arithmetic, but not its 400 loads, across the store -- and spills)
    int f = c.apply_scaling ? sc + s3 : 0; // the class's fact_sum_scale
    if (f > 1024)
    {
      f = 1023;
      *warn = 1;
    }
    const double x = regraft_product<S>(Ms + 2 * SS, o, y, pis, sub_left); // ... and its unscaled_site_lk_cat
    const double u = mix_unscale(x, f);
    site_lk += u * c.proba * c.r_w / q.head->r_sum * c.e_w / q.head->e_sum / q.head->sum_probas;
  }

  double contrib = 0.0;
  if (act)
  {
    const MixRegraftHead &h = *q.head;
    if (h.invar)
    { // src/mixt.c:1086-1116: Invariant_Lk of the invariant class at scale 2^0, then the mixing
      const int    iv = h.invar[p];
      const double inv = iv >= 0 ? h.pi_inv[iv] : 0.0;
      site_lk = site_lk * (1. - h.pinvar) + inv * h.pinvar;
    }
    if (site_lk < kSmall)
    {
      site_lk = kSmall;
      *warn = 1;
    }
    contrib = w * phyhip_log_ref(site_lk, phyhip_log_data); // src/mixt.c:1133
  }

  // the wave's fixed shuffle tree, then the waves in wave order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) contrib += __shfl_down(contrib, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) q.tile_sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// What scan_chunks (phyhip_scan.hpp) calls per chunk, for either scan: the matrix kernel over (distinct lengths, matrices per slot),
// the scan kernel over (tiles, candidates), the sums.  PQ / Q: the two parameter structs of the scan; they name these members alike.
template <class PQ, class Q>
static auto scan_launcher(hipStream_t stream, void (*pmat)(PQ), void (*scan)(Q), PQ &pq, Q &q, int per_slot, size_t tiles)
{
  return [=, &pq, &q](size_t n, size_t n_lengths, int keep_cand, const RegraftRec *d_recs, const double *d_lengths, int *d_flags, double *d_out) {
    q.recs = d_recs; q.keep_cand = keep_cand;
    pq.lengths = d_lengths; pq.flags = d_flags; pq.n_flags = (int)n;
    hipLaunchKernelGGL(pmat, dim3((unsigned)n_lengths, (unsigned)per_slot), dim3(256), 0, stream, pq);
    hipLaunchKernelGGL(scan, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, stream, q);
    hipLaunchKernelGGL(regraft_sum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, (const double *)q.tile_sums, d_out, (int)tiles, (int)n);
    return 0;
  };
}

// One plain instance: its patterns of every candidate.  sums[k] / warns[k] receive this instance's share.
static int regraft_run(Instance *I, int eigen, const phyhip_regraft_candidate *cand, int count, int keep, double *sums, int *warns)
{
  static const char *const who = "phyhip_calculate_regraft_log_likelihoods";
  int rc;
  if ((rc = refuse_kind(I, who, kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop | kRefuseStates))) return rc;
  if (I->C < 1 || I->C > kRegraftMaxCategories) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d categories", who, I->C);
  if (eigen < 0 || eigen >= I->NE) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: eigenIndex %d (0..%d)", who, eigen, I->NE - 1);
  if ((rc = regraft_check_candidates(I, cand, count, who))) return rc;
  RegraftUnit &U = side_of(I).regraft;
  U.valid = false;
  if ((rc = regraft_make_real(I, cand, count))) return rc;
  if ((rc = scan_reserve(U, I, I->C, 0, count, who))) return rc;
  const ScanLayout &L = U.lay;
  const size_t      SS = (size_t)I->S * I->S;
  RegraftParams     q;
  memset(&q, 0, sizeof q);
  q.keep = U.work.at<double>(L.keep); q.mats = U.work.at<double>(L.mats); q.tile_sums = U.work.at<double>(L.tile_sums);
  q.tip_codes = I->d_tipcodes; q.code_masks = I->d_masks; q.wght = I->d_wght; q.pi = I->d_pi; q.cat_w = I->d_catw; q.invar = I->invar_model ? I->d_invar : nullptr;
  q.partials = I->d_partials; q.scales = I->d_scales;
  q.P = I->P; q.Ppad = I->Ppad; q.C = I->C; q.tips = I->tips;
  q.apply_scaling = I->apply_scaling; q.pinvar = I->pinvar;
  RegraftPmatParams pq;
  memset(&pq, 0, sizeof pq);
  pq.mats = U.work.at<double>(L.mats); pq.C = I->C;
  pq.U = I->d_evec + (size_t)eigen * SS; pq.V = I->d_ivec + (size_t)eigen * SS; pq.R = I->d_eval + (size_t)eigen * I->S; pq.rates = I->d_catr;
  pq.br_len_mult = I->br_len_mult; pq.l_min = I->l_min; pq.l_max = I->l_max;
  const int  layout = layout_of(I);
  void (*pmat)(RegraftPmatParams) = regraft_pmat_kernel<4>;
  void (*scan)(RegraftParams) = layout == 2 ? regraft_scan_kernel<4, 2> : regraft_scan_kernel<4, 0>;
  if (I->S == 20) pmat = regraft_pmat_kernel<20>, scan = layout == 1 ? regraft_scan_kernel<20, 1> : regraft_scan_kernel<20, 0>;
  if ((rc = scan_chunks(U, I, cand, count, keep, sums, warns, nullptr, scan_launcher(I->stream, pmat, scan, pq, q, I->C, L.tiles)))) return rc;
  side_stream_drained(I); // the Lk(b) / dLk calls that follow can be served resident again
  return PHYHIP_SUCCESS;
}

// ---- the mixture scan's host side ----------------------------------------------------------------------------------------------------
struct MixRegraftCoef
{
  const double *proba, *r_w, *e_w;
  double        r_sum, e_sum, sum_probas;
};

// The class instances of one mixture (plain instances: the classes themselves, or one shard of each): their patterns of every
// candidate.  sums[k] / warns[k] receive this list's share.
static int mixregraft_run(const int *ids, int n_cls, const int *eigen, const phyhip_regraft_candidate *cand, int count, int keep,
                          const MixRegraftCoef &co, double *sums, int *warns)
{
  static const char *const who = "phyhip_calculate_mixture_regraft_log_likelihoods";
  int rc;
  std::vector<std::unique_ptr<Entered<false>>> entered; // (kSideCall: the large-grid resident workgroups of every class leave)
  std::vector<Instance *>                      cls;
  for (int k = 0; k < n_cls; ++k)
  {
    entered.emplace_back(new Entered<false>(ids[k]));
    if (entered.back()->rc()) return entered.back()->rc();
    cls.push_back(entered.back()->inst());
  }
  Instance *const I0 = cls[0];
  const int       layout = layout_of(I0);
  for (int k = 0; k < n_cls; ++k)
  {
    const Instance *I = cls[k];
    if ((rc = refuse_kind(I, who, kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop | kRefuseStates))) return rc;
    if (I->C != 1) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d has %d categories (a class instance has one)", who, k, I->C);
    if (I->P != I0->P || I->Ppad != I0->Ppad || I->S != I0->S || I->dev != I0->dev || I->tips != I0->tips || I->nbuf != I0->nbuf ||
        layout_of(I) != layout)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d: another pattern count, state count, buffer layout or device than class 0", who, k);
    if (eigen[k] < 0 || eigen[k] >= I->NE) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d: eigenIndex %d (0..%d)", who, k, eigen[k], I->NE - 1);
  }
  if ((rc = regraft_check_candidates(I0, cand, count, who))) return rc;
  RegraftUnit &U = side_of(I0).mixregraft;
  U.valid = false;
  // every class: its buffers real, its queue run, its stream drained -- all of it before anything is launched
  for (Instance *I : cls)
    if ((rc = regraft_make_real(I, cand, count))) return rc;
  if ((rc = scan_reserve(U, I0, n_cls, n_cls, count, who))) return rc;
  U.classes = n_cls;
  const ScanLayout &L = U.lay;
  // the head and the per-class table: they go up in front of every chunk's records
  const size_t SS = (size_t)I0->S * I0->S;
  MixRegraftHead head;
  memset(&head, 0, sizeof head);
  head.r_sum = co.r_sum; head.e_sum = co.e_sum; head.sum_probas = co.sum_probas;
  head.invar = I0->mix_invar_model ? I0->d_invar : nullptr; head.pinvar = I0->mix_pinvar;
  for (int s = 0; s < 20; ++s) head.pi_inv[s] = I0->mix_pi_inv[s];
  std::vector<MixRegraftClass> table((size_t)n_cls);
  for (int k = 0; k < n_cls; ++k)
  {
    const Instance  *I = cls[k];
    MixRegraftClass &t = table[k];
    memset(&t, 0, sizeof t);
    t.tip_codes = I->d_tipcodes; t.code_masks = I->d_masks; t.partials = I->d_partials; t.scales = I->d_scales; t.pi = I->d_pi;
    t.U = I->d_evec + (size_t)eigen[k] * SS; t.V = I->d_ivec + (size_t)eigen[k] * SS; t.R = I->d_eval + (size_t)eigen[k] * I->S;
    t.rate = I->h_rates[0]; t.br_len_mult = I->br_len_mult; t.l_min = I->l_min; t.l_max = I->l_max;
    t.proba = co.proba[k]; t.r_w = co.r_w[k]; t.e_w = co.e_w[k];
    t.apply_scaling = I->apply_scaling;
  }
  std::vector<char> prefix(L.prefix_bytes);
  memcpy(prefix.data(), &head, sizeof head);
  memcpy(prefix.data() + sizeof head, table.data(), (size_t)n_cls * sizeof(MixRegraftClass));
  MixRegraftParams q;
  memset(&q, 0, sizeof q);
  q.keep = U.work.at<double>(L.keep); q.mats = U.work.at<double>(L.mats); q.tile_sums = U.work.at<double>(L.tile_sums);
  q.head = U.work.at<MixRegraftHead>(L.prefix); q.cls = U.work.at<MixRegraftClass>(L.prefix + sizeof head);
  q.wght = I0->d_wght;
  q.P = I0->P; q.Ppad = I0->Ppad; q.n_cls = n_cls; q.tips = I0->tips;
  MixRegraftPmatParams pq;
  memset(&pq, 0, sizeof pq);
  pq.mats = U.work.at<double>(L.mats); pq.cls = q.cls; pq.n_cls = n_cls;
  void (*pmat)(MixRegraftPmatParams) = mixregraft_matrices_kernel<4>;
  void (*scan)(MixRegraftParams) = layout == 2 ? mixregraft_classes_kernel<4, 2> : mixregraft_classes_kernel<4, 0>;
  if (I0->S == 20) pmat = mixregraft_matrices_kernel<20>, scan = layout == 1 ? mixregraft_classes_kernel<20, 1> : mixregraft_classes_kernel<20, 0>;
  if ((rc = scan_chunks(U, I0, cand, count, keep, sums, warns, prefix.data(), scan_launcher(I0->stream, pmat, scan, pq, q, n_cls, L.tiles)))) return rc;
  for (Instance *I : cls) side_stream_drained(I); // every stream has drained
  return PHYHIP_SUCCESS;
}

// ---- what the entry points of the two scans share -------------------------------------------------------------------------------------
// a candidate's shard sums are added in shard order, its warnings ORed
struct __attribute__((visibility("hidden"))) ShardSums
{
  std::vector<double> part, sum;
  std::vector<int>    wpart, warn;
  explicit ShardSums(int count) : part((size_t)count), sum((size_t)count, 0.0), wpart((size_t)count), warn((size_t)count, 0) {}
  void add() { for (size_t k = 0; k < sum.size(); ++k) sum[k] += part[k], warn[k] |= wpart[k]; } // the shard that has just run
  void hand_over(double *outLogLikelihoods, int *outWarnings) const
  {
    std::copy(sum.begin(), sum.end(), outLogLikelihoods);
    if (outWarnings) std::copy(warn.begin(), warn.end(), outWarnings);
  }
};

static const char *const kScanCall = "phyhip_calculate_regraft_log_likelihoods call";
static const char *const kMixScanCall = "phyhip_calculate_mixture_regraft_log_likelihoods call with this first instance";

static int scan_left_something(const RegraftUnit &U, const char *who, const char *call)
{
  return U.valid && U.work.ptr ? 0 : fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no %s before it", who, call);
}

// the kept candidate's vector and exponents (of one class of a mixture scan), every shard its pattern range
static int scan_get_partials(int instance, RegraftUnit SideUnits::*unit, const char *who, const char *call, int classIndex, double *outPartials,
                             int *outScaleFactors)
{
  const bool mixture = unit == &SideUnits::mixregraft;
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long) {
    const RegraftUnit &U = side_of(I).*unit;
    if (const int rc = scan_left_something(U, who, call)) return rc;
    if (U.last_keep < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: the last call kept no candidate (keepCandidate -1)", who);
    if (mixture && (classIndex < 0 || classIndex >= U.classes)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d of %d", who, classIndex, U.classes);
    const size_t cls = mixture ? classIndex : 0, row = (size_t)(mixture ? 1 : I->C) * I->S; // (doubles of a pattern in the caller's array)
    if (outPartials) HIPCHK(hipMemcpy(outPartials + (size_t)lo * row, U.work.at<double>(U.lay.keep_of(cls)), U.lay.vec_bytes, hipMemcpyDeviceToHost));
    if (outScaleFactors) HIPCHK(hipMemcpy(outScaleFactors + lo, U.work.at<int>(U.lay.exps_of(cls)), (size_t)I->P * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  });
}

// one matrix of one candidate of the last chunk; classIndex: of a mixture scan, -1 of a plain one (all its categories)
static int scan_get_matrix(int instance, RegraftUnit SideUnits::*unit, const char *who, const char *call, int classIndex, int candidate, int which,
                           double *outMatrix)
{
  if (which < 0 || which > 2) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: which %d (0..2)", who, which);
  if (!outMatrix) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: outMatrix is NULL", who);
  const bool mixture = unit == &SideUnits::mixregraft;
  bool       done = false; // (the matrices are the same on every shard: the first one answers)
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    if (done) return 0;
    const RegraftUnit &U = side_of(I).*unit;
    if (const int rc = scan_left_something(U, who, call)) return rc;
    if (mixture && (classIndex < 0 || classIndex >= U.classes)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d of %d", who, classIndex, U.classes);
    if (candidate < 0 || candidate >= U.last_count) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d of %d", who, candidate, U.last_count);
    if (candidate < U.last_first)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d's matrices have left the work space (the call ran in %d chunks, the last from candidate %d)",
                  who, candidate, U.chunks, U.last_first);
    const size_t slot = (size_t)U.last_slots[3 * (size_t)(candidate - U.last_first) + which];
    HIPCHK(hipMemcpy(outMatrix, U.work.at<double>(U.lay.matrix(slot, mixture ? classIndex : 0)), mixture ? U.lay.mat_bytes : U.lay.slot_bytes,
                     hipMemcpyDeviceToHost));
    done = true;
    return 0;
  });
}

static int scan_set_work_space(int instance, RegraftUnit SideUnits::*unit, const char *who, long long maxBytes)
{
  if (maxBytes < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: %lld bytes", who, maxBytes);
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    (side_of(I).*unit).max_bytes = maxBytes ? (size_t)maxBytes : kRegraftWorkBytes;
    return 0;
  });
}

// read and reset: the time is added over the shards; calls and candidates are the same on every shard, the first one's are taken
static int scan_profile_read(int instance, RegraftUnit SideUnits::*unit, double *outKernelMs, int *outCalls, long long *outCandidates)
{
  double    ms = 0.0;
  int       n = 0;
  long long nc = 0;
  bool      first = true;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    RegraftUnit &U = side_of(I).*unit;
    ms += U.prof_ms;
    if (first) n = U.prof_n, nc = U.prof_cand;
    first = false;
    U.prof_ms = 0.0; U.prof_n = 0; U.prof_cand = 0;
    return 0;
  });
  if (rc < 0) return rc;
  if (outKernelMs) *outKernelMs = ms;
  if (outCalls) *outCalls = n;
  if (outCandidates) *outCandidates = nc;
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

int phyhip_calculate_regraft_log_likelihoods(int instance, int eigenIndex, const phyhip_regraft_candidate *candidates, int count, int keepCandidate,
                                             double *outLogLikelihoods, int *outWarnings)
{
  static const char *const who = "phyhip_calculate_regraft_log_likelihoods";
  if (count < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate count %d", who, count);
  if (count > 0 && (!candidates || !outLogLikelihoods)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: a NULL array for %d candidates", who, count);
  if (keepCandidate < -1 || keepCandidate >= count) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: keepCandidate %d of %d candidates", who, keepCandidate, count);
  if (count == 0)
  { // nothing runs: a plain instance is entered all the same, a group only reports a replay that failed while it drained
    if (Group *G = get_group(instance))
    {
      if (const int rc = group_take_drain_error(G)) return rc;
    }
    else
    {
      GET_INST(I, instance);
      (void)I;
    }
    return PHYHIP_SUCCESS;
  }
  // every shard scans its pattern range
  ShardSums s(count);
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    const int r = regraft_run(I, eigenIndex, candidates, count, keepCandidate, s.part.data(), s.wpart.data());
    if (r) return r;
    s.add();
    return 0;
  });
  if (rc < 0) return rc;
  s.hand_over(outLogLikelihoods, outWarnings);
  return PHYHIP_SUCCESS;
}

int phyhip_get_regraft_partials(int instance, double *outPartials, int *outScaleFactors)
{
  return scan_get_partials(instance, &SideUnits::regraft, "phyhip_get_regraft_partials", kScanCall, -1, outPartials, outScaleFactors);
}

int phyhip_get_regraft_transition_matrix(int instance, int candidate, int which, double *outMatrix)
{
  return scan_get_matrix(instance, &SideUnits::regraft, "phyhip_get_regraft_transition_matrix", kScanCall, -1, candidate, which, outMatrix);
}

int phyhip_set_regraft_work_space(int instance, long long maxBytes)
{
  return scan_set_work_space(instance, &SideUnits::regraft, "phyhip_set_regraft_work_space", maxBytes);
}

int phyhip_calculate_mixture_regraft_log_likelihoods(const int *instances, int count, const int *eigenIndices,
                                                     const phyhip_regraft_candidate *candidates, int candidateCount, int keepCandidate,
                                                     const double *classProba, const double *rMatWeight, const double *eFrqWeight,
                                                     double rMatWeightSum, double eFrqWeightSum, double sumProbas, double *outLogLikelihoods,
                                                     int *outWarnings)
{
  static const char *const who = "phyhip_calculate_mixture_regraft_log_likelihoods";
  if (count < 1 || count > kMaxMixClasses) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: %d mixture classes (1..%d)", who, count, kMaxMixClasses);
  if (!instances || !eigenIndices || !classProba || !rMatWeight || !eFrqWeight)
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: a NULL per-class array", who);
  if (candidateCount < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate count %d", who, candidateCount);
  if (candidateCount > 0 && (!candidates || !outLogLikelihoods))
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: a NULL array for %d candidates", who, candidateCount);
  if (keepCandidate < -1 || keepCandidate >= candidateCount)
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: keepCandidate %d of %d candidates", who, keepCandidate, candidateCount);
  const MixRegraftCoef co{classProba, rMatWeight, eFrqWeight, rMatWeightSum, eFrqWeightSum, sumProbas};
  Group *const G0 = get_group(instances[0]);
  if (!G0)
  {
    for (int k = 1; k < count; ++k)
      if (get_group(instances[k])) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d: sharded and plain class instances cannot be mixed", who, k);
    if (candidateCount == 0)
    { // nothing runs: the first instance is entered all the same
      GET_INST(I, instances[0]);
      (void)I;
      return PHYHIP_SUCCESS;
    }
    std::vector<int> warn((size_t)candidateCount, 0);
    if (const int rc = mixregraft_run(instances, count, eigenIndices, candidates, candidateCount, keepCandidate, co, outLogLikelihoods, warn.data()))
      return rc;
    if (outWarnings) std::copy(warn.begin(), warn.end(), outWarnings);
    return PHYHIP_SUCCESS;
  }
  // class instances that are one-process sharded instances of one shard layout: every shard scans its pattern range over its
  // sub-instances
  std::vector<Group *> Gs;
  int rc = mixture_groups(instances, count, Gs);
  if (rc) return rc;
  for (Group *G : Gs)
    if ((rc = group_take_drain_error(G))) return rc;
  if (candidateCount == 0) return PHYHIP_SUCCESS;
  ShardSums s(candidateCount);
  for (size_t g = 0; g < G0->sub_id.size(); ++g)
  {
    int ids[kMaxMixClasses];
    for (int k = 0; k < count; ++k) ids[k] = Gs[k]->sub_id[g];
    if ((rc = mixregraft_run(ids, count, eigenIndices, candidates, candidateCount, keepCandidate, co, s.part.data(), s.wpart.data()))) return rc;
    s.add();
  }
  s.hand_over(outLogLikelihoods, outWarnings);
  return PHYHIP_SUCCESS;
}

int phyhip_get_mixture_regraft_partials(int firstInstance, int classIndex, double *outPartials, int *outScaleFactors)
{
  return scan_get_partials(firstInstance, &SideUnits::mixregraft, "phyhip_get_mixture_regraft_partials", kMixScanCall, classIndex, outPartials,
                           outScaleFactors);
}

int phyhip_get_mixture_regraft_transition_matrix(int firstInstance, int classIndex, int candidate, int which, double *outMatrix)
{
  return scan_get_matrix(firstInstance, &SideUnits::mixregraft, "phyhip_get_mixture_regraft_transition_matrix", kMixScanCall, classIndex, candidate,
                         which, outMatrix);
}

int phyhip_set_mixture_regraft_work_space(int firstInstance, long long maxBytes)
{
  return scan_set_work_space(firstInstance, &SideUnits::mixregraft, "phyhip_set_mixture_regraft_work_space", maxBytes);
}

int phyhip_profile_read_mixture_regraft(int firstInstance, double *outKernelMs, int *outCalls, long long *outCandidates)
{
  return scan_profile_read(firstInstance, &SideUnits::mixregraft, outKernelMs, outCalls, outCandidates);
}

int phyhip_profile_read_regraft(int instance, double *outKernelMs, int *outCalls, long long *outCandidates)
{
  return scan_profile_read(instance, &SideUnits::regraft, outKernelMs, outCalls, outCandidates);
}

} // extern "C"
