// phyhip_regraft_dev.hpp -- the device functions a candidate of a regraft scan is made of, shared by the units that join three
// existing vectors per candidate (phyhip_regraft.hip: the plain and the mixture scan; phyhip_triple.hip: Triple_Dist): the matrix
// of one (length, category), one operand, the joined vector before the scaling decision, Lk_Core's product.  Device code and the
// plain structs it reads; no kernels.
#pragma once
#include "phyhip_side.hpp"
#include "phyhip_scan_plan.hpp" // RegraftRec, the record a scan kernel reads
#include "phyhip_layout.hpp"
#include "phyhip_log.hpp"

namespace phyhip_host
{

// what site_tail reads (phyhip_tail.hpp); the per-site outputs are not stored
struct RegraftTailQ
{
  const short  *invar;
  const double *pi;
  double       *site_lnl, *site_lk;
  int          *fact, *warn;
  int           invar_model, apply_scaling;
  double        pinvar;
};
struct NoStore
{
  template <class T> __device__ __forceinline__ void operator()(T *, const T) const {}
};

// PMat_Empirical of one (length, category) by one workgroup of 256: out[S][S] from the eigen system {U, V, R}
// (the entry loops stride by 256: a larger workgroup writes every entry, and writes it once, only where S * S <= 256 -- the callers
// with another workgroup size assert it)
template <int S>
__device__ __forceinline__ void regraft_pmat_body(const double l, const double *__restrict__ U, const double *__restrict__ V,
                                                  const double *__restrict__ R, const double rate, const double br_len_mult, const double l_min,
                                                  const double l_max, double *__restrict__ out, double *expt, double *tmp, double *rsum)
{
  const int tid = threadIdx.x;
  if (tid < S)
  {
    double len = (l > 0.0 ? l : 0.0) * rate; // src/lk.c:2296
    len *= br_len_mult;                      // :2297
    if (len < l_min) len = l_min;            // :2299-2300
    else if (len > l_max) len = l_max;
    expt[tid] = dev_exp(R[tid] * len);       // src/models.c:275
  }
  __syncthreads();
  // acc = sum_k (U[i][k] * expt[k]) * V[k][j], ascending k with FMA (src/models.c:278-292), then the floor (:293)
  for (int e = tid; e < S * S; e += 256)
  {
    const int i = e / S, j = e % S;
    double    acc = 0.0;
#pragma unroll
    for (int k = 0; k < S; ++k) acc = __builtin_fma(U[i * S + k] * expt[k], V[k * S + j], acc);
    tmp[e] = (acc < kSmallPij) ? kSmallPij : acc;
  }
  __syncthreads();
  if (tid < S)
  { // row sums in ascending j (:296-297)
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) sum += tmp[tid * S + j];
    rsum[tid] = sum;
  }
  __syncthreads();
  for (int e = tid; e < S * S; e += 256) out[e] = tmp[e] / rsum[e / S]; // :298
}

// one operand of category c at pattern p: a tip's 0/1 vector from its allowed-state mask, or a partials buffer in the instance's layout
// (Q: RegraftParams, or the class of a mixture scan as MixRegraftSrc names its buffers)
template <int S, int L, class Q>
__device__ __forceinline__ void regraft_operand(const Q &q, const int idx, const uint32_t mask, const long long p, const int c,
                                                double (&x)[S])
{
  if (idx < q.tips)
  {
#pragma unroll
    for (int j = 0; j < S; ++j) x[j] = ((mask >> j) & 1u) ? 1.0 : 0.0;
  }
  else
  {
#pragma unroll
    for (int j = 0; j < S; ++j) x[j] = q.partials[partial_off<S>(L, q.P, q.Ppad, q.C, idx - q.tips, p, c, j)];
  }
}

// the C*S values of one category before the scaling decision (src/avx.c:527-587)
template <int S, int L, class Q>
__device__ __forceinline__ void regraft_join(const Q &q, const RegraftRec &r, const uint32_t k1, const uint32_t k2, const long long p,
                                             const int c, const double *__restrict__ M1, const double *__restrict__ M2, double (&o)[S])
{
  double x1[S], x2[S];
  regraft_operand<S, L>(q, r.c1, k1, p, c, x1);
  regraft_operand<S, L>(q, r.c2, k2, p, c, x2);
  int ones = 1; // the all-ones shortcut of the Inin kernel (src/avx.c:575-587); (`&`, not `&&`: no chain of 2 S nested branches)
#pragma unroll
  for (int j = 0; j < S; ++j) ones &= (int)(x1[j] == 1.0) & (int)(x2[j] == 1.0);
  // u[i] = M[i][0] x[0], then the fused chain over ascending j (src/avx.c:593-616; matvec_rows of phyhip_kernels.hpp, every row
  // unrolled so that no array of a lane is indexed at run time)
#pragma unroll
  for (int i = 0; i < S; ++i)
  {
    double a = M1[i * S] * x1[0], b = M2[i * S] * x2[0];
#pragma unroll
    for (int j = 1; j < S; ++j)
    {
      a = __builtin_fma(M1[i * S + j], x1[j], a);
      b = __builtin_fma(M2[i * S + j], x2[j], b);
    }
    o[i] = ones ? 1.0 : a * b;
  }
}

// Lk_Core's product of one category (src/avx.c:130-148, 184-210): o the computed vector, y the subtree's, M3 the third matrix (rows:
// the right-side state); with sub_left the subtree is the left operand
template <int S>
__device__ __forceinline__ double regraft_product(const double *__restrict__ M3, const double (&o)[S], const double (&y)[S], const double *pis,
                                                  const bool sub_left)
{
  double lkc = 0.0;
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
      for (int i = 0; i < S; ++i) a = __builtin_fma(M3[k * S + i], sub_left ? y[i] : o[i], a);
      t[kk] = a * ((sub_left ? o[k] : y[k]) * pis[k]);
    }
    const double nrm = (t[0] + t[2]) + (t[1] + t[3]);
    lkc = (S == 4) ? nrm : lkc + nrm;
  }
  return lkc;
}

// what regraft_operand reads of one class of a mixture scan, or of one plain instance
struct MixRegraftSrc
{
  const double *partials;
  long long     P, Ppad;
  int           C, tips;
};

} // namespace phyhip_host
