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
#include <memory>

#include "phyhip_regraft_dev.hpp" // the matrix body, operand fetch, joined vector and product: shared with phyhip_triple.hip

namespace phyhip_host
{

constexpr int kRegraftMaxCategories = 8; // the 4-state kernel holds C * S values in registers
constexpr int kRegraftTile = 256;

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

// bytes of the work space one candidate of a chunk takes (its three matrices, tile sums, record, lengths, sum and flag) ...
static size_t regraft_candidate_bytes(const Instance *I)
{
  const size_t tiles = (size_t)((I->P + kRegraftTile - 1) / kRegraftTile);
  return 3 * (size_t)I->C * I->S * I->S * sizeof(double) + tiles * sizeof(double) + sizeof(RegraftRec) + 3 * sizeof(double) + sizeof(double) + 8;
}
// ... and of the kept vector with its exponents, which every call's layout reserves
static size_t regraft_keep_bytes(const Instance *I) { return (size_t)I->P * I->C * I->S * sizeof(double) + (((size_t)I->P + 1) & ~(size_t)1) * sizeof(int); }

// One plain instance: its patterns of every candidate.  sums[k] / warns[k] receive this instance's share.
static int regraft_run(Instance *I, int eigen, const phyhip_regraft_candidate *cand, int count, int keep, double *sums, int *warns)
{
  static const char *const who = "phyhip_calculate_regraft_log_likelihoods";
  int rc;
  if ((rc = refuse_kind(I, who, kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop | kRefuseStates))) return rc;
  if (I->C < 1 || I->C > kRegraftMaxCategories) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d categories", who, I->C);
  if (eigen < 0 || eigen >= I->NE) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: eigenIndex %d (0..%d)", who, eigen, I->NE - 1);
  for (int k = 0; k < count; ++k)
  {
    const phyhip_regraft_candidate &c = cand[k];
    if ((rc = check_partial_index(I, c.child1Partials, true)) || (rc = check_partial_index(I, c.child2Partials, true)) ||
        (rc = check_partial_index(I, c.subtreePartials, true)))
      return fail(rc, "%s: candidate %d: %s", who, k, std::string(g_err).c_str());
    if ((c.flags & PHYHIP_REGRAFT_SUBTREE_IS_LEFT) && c.subtreePartials < I->tips)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d: tip %d as the left operand", who, k, c.subtreePartials);
  }
  auto &U = side_of(I).regraft;
  U.valid = false;
  for (int k = 0; k < count; ++k)
  {
    devirtualise(I, cand[k].child1Partials); devirtualise(I, cand[k].child2Partials); devirtualise(I, cand[k].subtreePartials);
  }
  if ((rc = flush_sync(I))) return rc; // (queued matrix work and partial updates first: the path updates of the caller are seen)
  if ((rc = upload_masks(I))) return rc;

  const size_t SS = (size_t)I->S * I->S, MS = (size_t)I->C * SS, tiles = (size_t)((I->P + kRegraftTile - 1) / kRegraftTile);
  const size_t per = regraft_candidate_bytes(I), fixed = regraft_keep_bytes(I);
  size_t       chunk = U.max_bytes > fixed + per ? (U.max_bytes - fixed) / per : 1;
  chunk = std::min(chunk, std::min((size_t)count, (size_t)65535)); // (a grid's second dimension holds 65535 candidates)
  if ((rc = U.work.reserve(fixed + chunk * per, who))) return rc;
  // layout: kept vector | its exponents | matrices | of a launch of n: tile sums, flags (8 bytes per candidate), sums | records, lengths
  // (what goes up is one copy, what comes down is one copy)
  RegraftParams q;
  memset(&q, 0, sizeof q);
  q.keep = (double *)U.work.ptr;
  double *d_mats = (double *)((char *)U.work.ptr + fixed);
  q.mats = d_mats;
  q.tile_sums = d_mats + 3 * chunk * MS;
  RegraftRec *d_recs = (RegraftRec *)(q.tile_sums + chunk * tiles + 2 * chunk);
  q.recs = d_recs;
  q.tip_codes = I->d_tipcodes; q.code_masks = I->d_masks; q.wght = I->d_wght; q.pi = I->d_pi; q.cat_w = I->d_catw; q.invar = I->invar_model ? I->d_invar : nullptr;
  q.partials = I->d_partials; q.scales = I->d_scales;
  q.P = I->P; q.Ppad = I->Ppad; q.C = I->C; q.tips = I->tips;
  q.apply_scaling = I->apply_scaling; q.pinvar = I->pinvar;
  RegraftPmatParams pq;
  memset(&pq, 0, sizeof pq);
  pq.mats = d_mats; pq.C = I->C;
  pq.U = I->d_evec + (size_t)eigen * SS; pq.V = I->d_ivec + (size_t)eigen * SS; pq.R = I->d_eval + (size_t)eigen * I->S; pq.rates = I->d_catr;
  pq.br_len_mult = I->br_len_mult; pq.l_min = I->l_min; pq.l_max = I->l_max;

  std::vector<RegraftRec> recs;
  std::vector<double>     lens;
  std::vector<char>       up;
  std::vector<double>     down;
  std::unordered_map<unsigned long long, int> slot_of; // a length's bits -> its matrix slot: identical lengths of a chunk are built once
  auto slot = [&](double l) {
    unsigned long long bits;
    memcpy(&bits, &l, sizeof bits);
    const auto it = slot_of.find(bits);
    if (it != slot_of.end()) return it->second;
    lens.push_back(l);
    return slot_of[bits] = (int)lens.size() - 1;
  };
  SideTimer tm(I);
  U.chunks = 0;
  for (size_t first = 0; first < (size_t)count; first += chunk)
  {
    const size_t n = std::min(chunk, (size_t)count - first);
    recs.clear(); lens.clear(); slot_of.clear();
    for (size_t k = 0; k < n; ++k)
    {
      const phyhip_regraft_candidate &c = cand[first + k];
      recs.push_back(RegraftRec{c.child1Partials, c.child2Partials, c.subtreePartials, c.flags, slot(c.child1Length), slot(c.child2Length),
                                slot(c.subtreeLength), 0});
    }
    up.resize(n * sizeof(RegraftRec) + lens.size() * sizeof(double));
    memcpy(up.data(), recs.data(), n * sizeof(RegraftRec));
    memcpy(up.data() + n * sizeof(RegraftRec), lens.data(), lens.size() * sizeof(double));
    HIPCHK(hipMemcpyAsync(d_recs, up.data(), up.size(), hipMemcpyHostToDevice, I->stream));
    pq.lengths = (const double *)(d_recs + n);
    double *const d_down = q.tile_sums + n * tiles; // (where the scan kernel of a launch of n candidates looks for its flags)
    double *const d_out = d_down + n;
    pq.flags = (int *)d_down; pq.n_flags = (int)n;
    q.keep_cand = (keep >= (int)first && keep < (int)(first + n)) ? keep - (int)first : -1;
    if ((rc = tm.tic())) return rc;
    const dim3 pgrid((unsigned)lens.size(), (unsigned)I->C), sgrid((unsigned)tiles, (unsigned)n), block(256);
    const int layout = layout_of(I);
    if (I->S == 4)
    {
      hipLaunchKernelGGL(regraft_pmat_kernel<4>, pgrid, block, 0, I->stream, pq);
      if (layout == 2) hipLaunchKernelGGL((regraft_scan_kernel<4, 2>), sgrid, block, 0, I->stream, q);
      else hipLaunchKernelGGL((regraft_scan_kernel<4, 0>), sgrid, block, 0, I->stream, q);
    }
    else
    {
      hipLaunchKernelGGL(regraft_pmat_kernel<20>, pgrid, block, 0, I->stream, pq);
      if (layout == 1) hipLaunchKernelGGL((regraft_scan_kernel<20, 1>), sgrid, block, 0, I->stream, q);
      else hipLaunchKernelGGL((regraft_scan_kernel<20, 0>), sgrid, block, 0, I->stream, q);
    }
    hipLaunchKernelGGL(regraft_sum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, I->stream, (const double *)q.tile_sums, d_out, (int)tiles,
                       (int)n);
    HIPCHK(hipGetLastError());
    if ((rc = tm.mark())) return rc;
    HIPCHK(hipStreamSynchronize(I->stream));
    if ((rc = tm.toc(U.prof_ms))) return rc;
    down.resize(2 * n);
    HIPCHK(hipMemcpy(down.data(), d_down, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
    memcpy(sums + first, down.data() + n, n * sizeof(double));
    for (size_t k = 0; k < n; ++k) warns[first + k] = reinterpret_cast<const int *>(down.data())[k] ? 1 : 0;
    ++U.chunks;
    U.last_first = (int)first;
  }
  // the last chunk's matrices stay in the work space for phyhip_get_regraft_transition_matrix
  U.last_slots.resize(recs.size() * 3);
  for (size_t k = 0; k < recs.size(); ++k)
  {
    U.last_slots[3 * k] = recs[k].m1; U.last_slots[3 * k + 1] = recs[k].m2; U.last_slots[3 * k + 2] = recs[k].m3;
  }
  U.last_count = count; U.last_keep = keep; U.valid = true;
  if (I->prof)
  {
    ++U.prof_n;
    U.prof_cand += count;
  }
  // the stream has drained: clean at once -- the Lk(b) / dLk calls that follow can be served resident again
  I->stream_dirty = false; I->clean_after = 0; ++I->clean_epoch;
  return PHYHIP_SUCCESS;
}

// ---- the mixture scan's host side ----------------------------------------------------------------------------------------------------
static size_t mixregraft_exponent_ints(const Instance *I) { return ((size_t)I->P + 1) & ~(size_t)1; }
// bytes of the work space one candidate of a chunk takes over n classes ...
static size_t mixregraft_candidate_bytes(const Instance *I, int n)
{
  const size_t tiles = (size_t)((I->P + kRegraftTile - 1) / kRegraftTile);
  return 3 * (size_t)n * I->S * I->S * sizeof(double) + tiles * sizeof(double) + sizeof(RegraftRec) + 3 * sizeof(double) + sizeof(double) + 8;
}
// ... and of the kept vectors with their exponents and the per-class table, which every call's layout reserves
static size_t mixregraft_keep_bytes(const Instance *I, int n) { return (size_t)n * ((size_t)I->P * I->S * sizeof(double) + mixregraft_exponent_ints(I) * sizeof(int)); }
static size_t mixregraft_table_bytes(int n) { return sizeof(MixRegraftHead) + (size_t)n * sizeof(MixRegraftClass); } // (the head in front of the table)
static size_t mixregraft_fixed_bytes(const Instance *I, int n) { return mixregraft_keep_bytes(I, n) + mixregraft_table_bytes(n); }

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
  for (int k = 0; k < count; ++k)
  {
    const phyhip_regraft_candidate &c = cand[k];
    if ((rc = check_partial_index(I0, c.child1Partials, true)) || (rc = check_partial_index(I0, c.child2Partials, true)) ||
        (rc = check_partial_index(I0, c.subtreePartials, true)))
      return fail(rc, "%s: candidate %d: %s", who, k, std::string(g_err).c_str());
    if ((c.flags & PHYHIP_REGRAFT_SUBTREE_IS_LEFT) && c.subtreePartials < I0->tips)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d: tip %d as the left operand", who, k, c.subtreePartials);
  }
  auto &U = side_of(I0).mixregraft;
  U.valid = false;
  // every class: the buffers a record names stored, queued matrix work and partial updates run (the path updates of the caller are
  // seen), its stream drained -- all of it before anything is launched
  for (Instance *I : cls)
  {
    for (int k = 0; k < count; ++k)
    {
      devirtualise(I, cand[k].child1Partials); devirtualise(I, cand[k].child2Partials); devirtualise(I, cand[k].subtreePartials);
    }
    if ((rc = flush_sync(I))) return rc;
    if ((rc = upload_masks(I))) return rc;
  }

  const size_t SS = (size_t)I0->S * I0->S, MS = (size_t)n_cls * SS, tiles = (size_t)((I0->P + kRegraftTile - 1) / kRegraftTile);
  const size_t per = mixregraft_candidate_bytes(I0, n_cls), fixed = mixregraft_fixed_bytes(I0, n_cls);
  size_t       chunk = U.max_bytes > fixed + per ? (U.max_bytes - fixed) / per : 1;
  chunk = std::min(chunk, std::min((size_t)count, (size_t)65535)); // (a grid's second dimension holds 65535 candidates)
  if ((rc = U.work.reserve(fixed + chunk * per, who))) return rc;
  // layout: kept vectors | their exponents | matrices | of a launch of n: tile sums, flags (8 bytes per candidate), sums | class table,
  // records, lengths (what goes up is one copy, what comes down is one copy)
  MixRegraftParams q;
  memset(&q, 0, sizeof q);
  q.keep = (double *)U.work.ptr;
  double *d_mats = (double *)((char *)U.work.ptr + mixregraft_keep_bytes(I0, n_cls));
  q.mats = d_mats;
  q.tile_sums = d_mats + 3 * chunk * MS;
  MixRegraftHead  *d_head = (MixRegraftHead *)(q.tile_sums + chunk * tiles + 2 * chunk);
  MixRegraftClass *d_cls = (MixRegraftClass *)(d_head + 1);
  RegraftRec      *d_recs = (RegraftRec *)(d_cls + n_cls);
  q.head = d_head; q.cls = d_cls; q.recs = d_recs;
  q.wght = I0->d_wght;
  q.P = I0->P; q.Ppad = I0->Ppad; q.n_cls = n_cls; q.tips = I0->tips;
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
  MixRegraftPmatParams pq;
  memset(&pq, 0, sizeof pq);
  pq.mats = d_mats; pq.cls = d_cls; pq.n_cls = n_cls;

  std::vector<RegraftRec> recs;
  std::vector<double>     lens;
  std::vector<char>       up;
  std::vector<double>     down;
  std::unordered_map<unsigned long long, int> slot_of; // a length's bits -> its matrix slot: identical lengths of a chunk are built once per class
  auto slot = [&](double l) {
    unsigned long long bits;
    memcpy(&bits, &l, sizeof bits);
    const auto it = slot_of.find(bits);
    if (it != slot_of.end()) return it->second;
    lens.push_back(l);
    return slot_of[bits] = (int)lens.size() - 1;
  };
  SideTimer tm(I0);
  U.chunks = 0;
  const size_t tb = mixregraft_table_bytes(n_cls);
  for (size_t first = 0; first < (size_t)count; first += chunk)
  {
    const size_t n = std::min(chunk, (size_t)count - first);
    recs.clear(); lens.clear(); slot_of.clear();
    for (size_t k = 0; k < n; ++k)
    {
      const phyhip_regraft_candidate &c = cand[first + k];
      recs.push_back(RegraftRec{c.child1Partials, c.child2Partials, c.subtreePartials, c.flags, slot(c.child1Length), slot(c.child2Length),
                                slot(c.subtreeLength), 0});
    }
    up.resize(tb + n * sizeof(RegraftRec) + lens.size() * sizeof(double));
    memcpy(up.data(), &head, sizeof head);
    memcpy(up.data() + sizeof head, table.data(), (size_t)n_cls * sizeof(MixRegraftClass));
    memcpy(up.data() + tb, recs.data(), n * sizeof(RegraftRec));
    memcpy(up.data() + tb + n * sizeof(RegraftRec), lens.data(), lens.size() * sizeof(double));
    HIPCHK(hipMemcpyAsync(d_head, up.data(), up.size(), hipMemcpyHostToDevice, I0->stream));
    pq.lengths = (const double *)(d_recs + n);
    double *const d_down = q.tile_sums + n * tiles; // (where the scan kernel of a launch of n candidates looks for its flags)
    double *const d_out = d_down + n;
    pq.flags = (int *)d_down; pq.n_flags = (int)n;
    q.keep_cand = (keep >= (int)first && keep < (int)(first + n)) ? keep - (int)first : -1;
    if ((rc = tm.tic())) return rc;
    const dim3 pgrid((unsigned)lens.size(), (unsigned)n_cls), sgrid((unsigned)tiles, (unsigned)n), block(256);
    if (I0->S == 4)
    {
      hipLaunchKernelGGL(mixregraft_matrices_kernel<4>, pgrid, block, 0, I0->stream, pq);
      if (layout == 2) hipLaunchKernelGGL((mixregraft_classes_kernel<4, 2>), sgrid, block, 0, I0->stream, q);
      else hipLaunchKernelGGL((mixregraft_classes_kernel<4, 0>), sgrid, block, 0, I0->stream, q);
    }
    else
    {
      hipLaunchKernelGGL(mixregraft_matrices_kernel<20>, pgrid, block, 0, I0->stream, pq);
      if (layout == 1) hipLaunchKernelGGL((mixregraft_classes_kernel<20, 1>), sgrid, block, 0, I0->stream, q);
      else hipLaunchKernelGGL((mixregraft_classes_kernel<20, 0>), sgrid, block, 0, I0->stream, q);
    }
    hipLaunchKernelGGL(regraft_sum_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, I0->stream, (const double *)q.tile_sums, d_out, (int)tiles,
                       (int)n);
    HIPCHK(hipGetLastError());
    if ((rc = tm.mark())) return rc;
    HIPCHK(hipStreamSynchronize(I0->stream));
    if ((rc = tm.toc(U.prof_ms))) return rc;
    down.resize(2 * n);
    HIPCHK(hipMemcpy(down.data(), d_down, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
    memcpy(sums + first, down.data() + n, n * sizeof(double));
    for (size_t k = 0; k < n; ++k) warns[first + k] = reinterpret_cast<const int *>(down.data())[k] ? 1 : 0;
    ++U.chunks;
    U.last_first = (int)first;
  }
  // the last chunk's matrices stay in the work space for phyhip_get_mixture_regraft_transition_matrix
  U.last_slots.resize(recs.size() * 3);
  for (size_t k = 0; k < recs.size(); ++k)
  {
    U.last_slots[3 * k] = recs[k].m1; U.last_slots[3 * k + 1] = recs[k].m2; U.last_slots[3 * k + 2] = recs[k].m3;
  }
  U.classes = n_cls; U.last_count = count; U.last_keep = keep; U.valid = true;
  if (I0->prof)
  {
    ++U.prof_n;
    U.prof_cand += count;
  }
  // every stream has drained: clean at once -- the Lk(b) / dLk calls that follow can be served resident again
  for (Instance *I : cls)
  {
    I->stream_dirty = false; I->clean_after = 0; ++I->clean_epoch;
  }
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
  // every shard scans its pattern range; a candidate's shard sums are added here in shard order
  std::vector<double> part((size_t)count), sum((size_t)count, 0.0);
  std::vector<int>    wpart((size_t)count), warn((size_t)count, 0);
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    const int r = regraft_run(I, eigenIndex, candidates, count, keepCandidate, part.data(), wpart.data());
    if (r) return r;
    for (int k = 0; k < count; ++k)
    {
      sum[k] += part[k];
      warn[k] |= wpart[k];
    }
    return 0;
  });
  if (rc < 0) return rc;
  for (int k = 0; k < count; ++k) outLogLikelihoods[k] = sum[k];
  if (outWarnings)
    for (int k = 0; k < count; ++k) outWarnings[k] = warn[k];
  return PHYHIP_SUCCESS;
}

int phyhip_get_regraft_partials(int instance, double *outPartials, int *outScaleFactors)
{
  static const char *const who = "phyhip_get_regraft_partials";
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long) {
    auto &U = side_of(I).regraft;
    if (!U.valid || !U.work.ptr) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no phyhip_calculate_regraft_log_likelihoods call before it", who);
    if (U.last_keep < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: the last call kept no candidate (keepCandidate -1)", who);
    const size_t  CS = (size_t)I->C * I->S;
    const double *d_keep = (const double *)U.work.ptr;
    if (outPartials) HIPCHK(hipMemcpy(outPartials + (size_t)lo * CS, d_keep, (size_t)I->P * CS * sizeof(double), hipMemcpyDeviceToHost));
    if (outScaleFactors) HIPCHK(hipMemcpy(outScaleFactors + lo, d_keep + (size_t)I->P * CS, (size_t)I->P * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  });
}

int phyhip_get_regraft_transition_matrix(int instance, int candidate, int which, double *outMatrix)
{
  static const char *const who = "phyhip_get_regraft_transition_matrix";
  if (which < 0 || which > 2) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: which %d (0..2)", who, which);
  if (!outMatrix) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: outMatrix is NULL", who);
  bool done = false; // (the matrices are the same on every shard: the first one answers)
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    if (done) return 0;
    auto &U = side_of(I).regraft;
    if (!U.valid || !U.work.ptr) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no phyhip_calculate_regraft_log_likelihoods call before it", who);
    if (candidate < 0 || candidate >= U.last_count) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d of %d", who, candidate, U.last_count);
    if (candidate < U.last_first)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d's matrices have left the work space (the call ran in %d chunks, the last from candidate %d)",
                  who, candidate, U.chunks, U.last_first);
    const size_t  MS = (size_t)I->C * I->S * I->S;
    const double *d_mats = (const double *)((const char *)U.work.ptr + regraft_keep_bytes(I));
    HIPCHK(hipMemcpy(outMatrix, d_mats + (size_t)U.last_slots[3 * (size_t)(candidate - U.last_first) + which] * MS, MS * sizeof(double),
                     hipMemcpyDeviceToHost));
    done = true;
    return 0;
  });
}

int phyhip_set_regraft_work_space(int instance, long long maxBytes)
{
  if (maxBytes < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_set_regraft_work_space: %lld bytes", maxBytes);
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    side_of(I).regraft.max_bytes = maxBytes ? (size_t)maxBytes : kRegraftWorkBytes;
    return 0;
  });
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
    if (outWarnings)
      for (int k = 0; k < candidateCount; ++k) outWarnings[k] = warn[k];
    return PHYHIP_SUCCESS;
  }
  // class instances that are one-process sharded instances of one shard layout: every shard scans its pattern range over its
  // sub-instances; a candidate's shard sums are added here in shard order
  std::vector<Group *> Gs;
  int rc = mixture_groups(instances, count, Gs);
  if (rc) return rc;
  for (Group *G : Gs)
    if ((rc = group_take_drain_error(G))) return rc;
  if (candidateCount == 0) return PHYHIP_SUCCESS;
  std::vector<double> part((size_t)candidateCount), sum((size_t)candidateCount, 0.0);
  std::vector<int>    wpart((size_t)candidateCount), warn((size_t)candidateCount, 0);
  for (size_t g = 0; g < G0->sub_id.size(); ++g)
  {
    int ids[kMaxMixClasses];
    for (int k = 0; k < count; ++k) ids[k] = Gs[k]->sub_id[g];
    if ((rc = mixregraft_run(ids, count, eigenIndices, candidates, candidateCount, keepCandidate, co, part.data(), wpart.data()))) return rc;
    for (int k = 0; k < candidateCount; ++k)
    {
      sum[k] += part[k];
      warn[k] |= wpart[k];
    }
  }
  for (int k = 0; k < candidateCount; ++k) outLogLikelihoods[k] = sum[k];
  if (outWarnings)
    for (int k = 0; k < candidateCount; ++k) outWarnings[k] = warn[k];
  return PHYHIP_SUCCESS;
}

int phyhip_get_mixture_regraft_partials(int firstInstance, int classIndex, double *outPartials, int *outScaleFactors)
{
  static const char *const who = "phyhip_get_mixture_regraft_partials";
  return side_each<kSideDrain, kSideCall>(firstInstance, [&](Instance *I, long long lo, long long) {
    auto &U = side_of(I).mixregraft;
    if (!U.valid || !U.work.ptr)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no phyhip_calculate_mixture_regraft_log_likelihoods call with this first instance before it", who);
    if (U.last_keep < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: the last call kept no candidate (keepCandidate -1)", who);
    if (classIndex < 0 || classIndex >= U.classes) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d of %d", who, classIndex, U.classes);
    const size_t  PS = (size_t)I->P * I->S;
    const double *d_keep = (const double *)U.work.ptr;
    const int    *d_exp = reinterpret_cast<const int *>(d_keep + (size_t)U.classes * PS) + (size_t)classIndex * mixregraft_exponent_ints(I);
    if (outPartials) HIPCHK(hipMemcpy(outPartials + (size_t)lo * I->S, d_keep + (size_t)classIndex * PS, PS * sizeof(double), hipMemcpyDeviceToHost));
    if (outScaleFactors) HIPCHK(hipMemcpy(outScaleFactors + lo, d_exp, (size_t)I->P * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  });
}

int phyhip_get_mixture_regraft_transition_matrix(int firstInstance, int classIndex, int candidate, int which, double *outMatrix)
{
  static const char *const who = "phyhip_get_mixture_regraft_transition_matrix";
  if (which < 0 || which > 2) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: which %d (0..2)", who, which);
  if (!outMatrix) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: outMatrix is NULL", who);
  bool done = false; // (the matrices are the same on every shard: the first one answers)
  return side_each<kSideDrain, kSideCall>(firstInstance, [&](Instance *I, long long, long long) {
    if (done) return 0;
    auto &U = side_of(I).mixregraft;
    if (!U.valid || !U.work.ptr)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no phyhip_calculate_mixture_regraft_log_likelihoods call with this first instance before it", who);
    if (classIndex < 0 || classIndex >= U.classes) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: class %d of %d", who, classIndex, U.classes);
    if (candidate < 0 || candidate >= U.last_count) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d of %d", who, candidate, U.last_count);
    if (candidate < U.last_first)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d's matrices have left the work space (the call ran in %d chunks, the last from candidate %d)",
                  who, candidate, U.chunks, U.last_first);
    const size_t  SS = (size_t)I->S * I->S;
    const double *d_mats = (const double *)((const char *)U.work.ptr + mixregraft_keep_bytes(I, U.classes));
    const size_t  slot = (size_t)U.last_slots[3 * (size_t)(candidate - U.last_first) + which];
    HIPCHK(hipMemcpy(outMatrix, d_mats + (slot * U.classes + classIndex) * SS, SS * sizeof(double), hipMemcpyDeviceToHost));
    done = true;
    return 0;
  });
}

int phyhip_set_mixture_regraft_work_space(int firstInstance, long long maxBytes)
{
  if (maxBytes < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_set_mixture_regraft_work_space: %lld bytes", maxBytes);
  return side_each<kSideDrain, kSideCall>(firstInstance, [&](Instance *I, long long, long long) {
    side_of(I).mixregraft.max_bytes = maxBytes ? (size_t)maxBytes : kRegraftWorkBytes;
    return 0;
  });
}

int phyhip_profile_read_mixture_regraft(int firstInstance, double *outKernelMs, int *outCalls, long long *outCandidates)
{
  double    ms = 0.0;
  int       n = 0;
  long long nc = 0;
  bool      first = true; // (calls and candidates are the same on every shard; the time is added over the shards)
  const int rc = side_each<kSideDrain, kSideCall>(firstInstance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).mixregraft;
    ms += U.prof_ms;
    if (first)
    {
      n = U.prof_n;
      nc = U.prof_cand;
    }
    first = false;
    U.prof_ms = 0.0;
    U.prof_n = 0;
    U.prof_cand = 0;
    return 0;
  });
  if (rc < 0) return rc;
  if (outKernelMs) *outKernelMs = ms;
  if (outCalls) *outCalls = n;
  if (outCandidates) *outCandidates = nc;
  return PHYHIP_SUCCESS;
}

int phyhip_profile_read_regraft(int instance, double *outKernelMs, int *outCalls, long long *outCandidates)
{
  double    ms = 0.0;
  int       n = 0;
  long long nc = 0;
  bool      first = true; // (calls and candidates are the same on every shard; the time is added over the shards)
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).regraft;
    ms += U.prof_ms;
    if (first)
    {
      n = U.prof_n;
      nc = U.prof_cand;
    }
    first = false;
    U.prof_ms = 0.0;
    U.prof_n = 0;
    U.prof_cand = 0;
    return 0;
  });
  if (rc < 0) return rc;
  if (outKernelMs) *outKernelMs = ms;
  if (outCalls) *outCalls = n;
  if (outCandidates) *outCandidates = nc;
  return PHYHIP_SUCCESS;
}

} // extern "C"
