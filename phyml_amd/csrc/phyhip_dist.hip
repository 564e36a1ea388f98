// phyhip_dist.hip -- the pairwise maximum-likelihood distance matrix: phyhip_calculate_pairwise_ml_distances
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// ML_Dist (src/lk.c:1783-1906) is what a default run does before its first likelihood call: for every pair of taxa j < k, with one
// rate category of rate 1,
//   F[s0][s1] = sum of wght[p] over the patterns where BOTH tips have exactly one allowed state, len = sum F, F /= len
//   init      = K80_dist (4 states) / JC69_Dist (else) of the pair, src/utilities.c:2407-2587; 0.1 where that is < 0 or > DIST_MAX - SMALL
//   d         = init where sum F < .001, else Opt_Dist_F -> Dist_F_Brent (src/optimiz.c:1848-1972) on -Lk_Dist (src/lk.c:2416-2473)
//   d         = min(d, DIST_MAX)
// Three kinds of kernel, all FP64:
//   * dist_count_kernel: the raw counts of all pairs are X diag(w) X^T with X the (taxon, state) x pattern one-hot matrix read
//     straight from the tip rows (a tip whose state set is not one state: a zero column).  v_mfma_f64_16x16x4_f64: a wave owns a
//     16-row x 64-column strip of the result (four accumulator blocks) and walks ALL patterns in ascending order, so every output
//     has one fixed order of additions -- no split over patterns, no atomics: the same bits from run to run for any weights, and
//     exact sums for integer weights.  Rows and columns are the flattened index taxon * S + state, so 20 states waste no lanes.
//     The result is walked in bands of taxa (rows), the work space stays bounded; blocks wholly below the diagonal are skipped.
//   * dist_sums_kernel: per pair len and the transition / transversion (4 states) or mismatch (else) sums, each in a fixed order.
//     The starting values are formed from them ON THE HOST with libm's pow / log: the optimiser stops long before convergence, so
//     its answer follows its starting value one for one, and K80's formula multiplies pow's last bit by 5e5.
//   * dist_opt_kernel: one wave per pair.  PMat_Empirical's arithmetic as pmat_kernel has it (src/models.c:275-298: (U e) first,
//     the fused chain over ascending k, the SMALL_PIJ floor, the row sum over ascending j, the division), the reference libm's exp
//     and log, Lk_Dist's sum in its order (i < j terms with i outer, then the diagonal) with plain products and additions, and
//     Dist_F_Brent line by line.  Every lane of the wave holds the same scalars; the matrix work is spread over the lanes in LDS.
// The call writes a work space of its own: partials, scale vectors, matrices, the last evaluation's outputs and the numerical
// warning stay what they were, and nothing queued is flushed (tips and weights are set synchronously, the model in stream order).
#include "phyhip_side.hpp"
#include "phyhip_layout.hpp"
#include "phyhip_log.hpp"

namespace phyhip_host
{

constexpr double kDistMax = 2.0;           // DIST_MAX, src/utilities.h:351
constexpr int    kDistColTiles = 4;        // 16-column blocks per wave of dist_count_kernel
// (the raw counts of one band of taxa stay below SideUnits::dist.band_bytes: phyhip_set_pairwise_work_space)

typedef double dist_f64x4 __attribute__((ext_vector_type(4)));

struct DistCountParams
{
  const uint8_t  *tip_codes;
  const uint32_t *code_masks;
  const double   *wght;
  double         *G;   // [band rows padded to 16][ldg]: row r - row0, column c (flattened taxon * S + state)
  long long       P, Ppad;
  int             n, row0, ldg;
};

// the one state of tip `t` at pattern p, or -1 (several allowed states, or p beyond the alignment)
template <int S> __device__ __forceinline__ int dist_tip_state(const DistCountParams &q, int t, long long p)
{
  if (t >= q.n || p >= q.P) return -1;
  const uint32_t m = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, t, p);
  return __popc(m) == 1 ? __ffs((int)m) - 1 : -1;
}

// grid (ldg / 64, row blocks of the band), one wave per workgroup.  Operand maps of v_mfma_f64_16x16x4_f64: lane l holds
// A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15]; result register g of lane l is D[row (l >> 4) + 4 g][column l & 15].
template <int S> __global__ __launch_bounds__(64) void dist_count_kernel(const DistCountParams q)
{
  const int lane = threadIdx.x, lo = lane & 15, kq = lane >> 4;
  const int rloc = 16 * (int)blockIdx.y, r = q.row0 + rloc + lo; // this lane's A row
  const int ta = r / S, sa = r % S;
  const int c0 = 64 * (int)blockIdx.x;
  const int row_min_taxon = (q.row0 + rloc) / S;
  bool      live[kDistColTiles];
  int       tb[kDistColTiles], sb[kDistColTiles];
  bool      any = false;
#pragma unroll
  for (int x = 0; x < kDistColTiles; ++x)
  {
    const int c = c0 + 16 * x + lo;
    tb[x] = c / S; sb[x] = c % S;
    live[x] = (c0 + 16 * x + 15) / S > row_min_taxon; // (wave-uniform) some column taxon lies above some row taxon
    any = any || live[x];
  }
  if (!any) return;
  dist_f64x4 acc[kDistColTiles];
#pragma unroll
  for (int x = 0; x < kDistColTiles; ++x) acc[x] = dist_f64x4{0.0, 0.0, 0.0, 0.0};

  for (long long p0 = 0; p0 < q.P; p0 += 16)
  {
    double a[4], b[kDistColTiles][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
      const long long p = p0 + 4 * i + kq;
      double          w = p < q.P ? q.wght[p] : 0.0;
      w = w > kSmall ? w : 0.0; // src/lk.c: a pattern of no weight is not there
      a[i] = dist_tip_state<S>(q, ta, p) == sa ? 1.0 : 0.0;
#pragma unroll
      for (int x = 0; x < kDistColTiles; ++x) b[x][i] = (live[x] && dist_tip_state<S>(q, tb[x], p) == sb[x]) ? w : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int x = 0; x < kDistColTiles; ++x)
        if (live[x]) acc[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[x][i], acc[x], 0, 0, 0);
  }
#pragma unroll
  for (int x = 0; x < kDistColTiles; ++x)
    if (live[x])
    {
#pragma unroll
      for (int g = 0; g < 4; ++g) q.G[(size_t)(rloc + kq + 4 * g) * q.ldg + (size_t)(c0 + 16 * x + lo)] = acc[x][g];
    }
}

// a sharded instance: the next shard's raw counts added to the first one's, element by element
__global__ __launch_bounds__(256) void dist_add_kernel(double *__restrict__ dst, const double *__restrict__ src, size_t n)
{
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = dst[i] + src[i];
}

struct DistPairParams
{
  const double *G;      // the band's raw counts
  double       *sums;   // [pair][3]: len, transitions | mismatches, transversions
  const double *init;   // [pair]: what K80_dist / JC69_Dist gave
  double       *dist, *lnl, *counts; // [pair], [pair], [pair of the band][S][S] or nullptr
  int          *iters;  // [pair]
  const double *U, *V, *R, *pi;
  double        l_min, l_max, min_diff_lk;
  int           n, j0, j1, ldg;
  long long     pair0;  // number of the band's first pair
};

__device__ __forceinline__ long long dist_pair_index(int n, int j, int k) { return (long long)j * n - (long long)j * (j + 1) / 2 + (k - j - 1); }

// grid (ceil(n / 256), taxa of the band): one lane per pair (j, k), k > j
template <int S> __global__ __launch_bounds__(256) void dist_sums_kernel(const DistPairParams q)
{
  const int j = q.j0 + (int)blockIdx.y, k = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (k <= j || k >= q.n) return;
  const double *g = q.G + (size_t)(j - q.j0) * S * q.ldg + (size_t)k * S;
  double len = 0.0, mis = 0.0, ts = 0.0;
#pragma unroll
  for (int s0 = 0; s0 < S; ++s0)
#pragma unroll
    for (int s1 = 0; s1 < S; ++s1)
    {
      const double v = g[(size_t)s0 * q.ldg + s1];
      len += v;
      // A, C, G, T = 0..3: A <-> G and C <-> T are the transitions
      if (S == 4 && (s0 ^ s1) == 2) ts += v;
      else if (s0 != s1) mis += v;
    }
  double *o = q.sums + 3 * dist_pair_index(q.n, j, k);
  o[0] = len;
  o[1] = S == 4 ? ts : mis;
  o[2] = S == 4 ? mis : 0.0;
}

template <int S> struct DistLds
{
  double U[S * S], V[S * S], F[S * S], T[S * S], e[S], rs[S], pi[S], R[S];
};

// Lk_Dist (src/lk.c:2416-2473) with one category of rate 1; every lane returns the same double
template <int S> __device__ __forceinline__ double dist_lk(DistLds<S> &L, const double dist, const double l_min, const double l_max, const int lane)
{
  double len = dist; // dist * gamma_rr[0], gamma_rr[0] == 1
  if (len < l_min) len = l_min;
  else if (len > l_max) len = l_max;
  __syncthreads(); // (the previous call's readers of T are through)
  if (lane < S) L.e[lane] = dev_exp(L.R[lane] * len); // src/models.c:275
  __syncthreads();
#pragma unroll 1
  for (int x = lane; x < S * S; x += 64)
  {
    const int i = x / S, j = x % S;
    double    acc = 0.0;
#pragma unroll
    for (int k = 0; k < S; ++k) acc = __builtin_fma(L.U[i * S + k] * L.e[k], L.V[k * S + j], acc); // :278-292
    L.T[x] = acc < kSmallPij ? kSmallPij : acc;                                                      // :293
  }
  __syncthreads();
  if (lane < S)
  {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) sum += L.T[lane * S + j]; // :296-297
    L.rs[lane] = sum;
  }
  __syncthreads();
#pragma unroll 1
  for (int x = lane; x < S * S; x += 64)
  {
    const int i = x / S, j = x % S;
    if (j >= i)
    {
      const double pij = L.T[x] / L.rs[i]; // :298
      const double f = i == j ? L.F[x] : L.F[i * S + j] + L.F[j * S + i];
      L.T[x] = f * phyhip_log_ref(L.pi[i] * pij, phyhip_log_data);
    }
  }
  __syncthreads();
  double lnL = 0.0;
#pragma unroll 1
  for (int i = 0; i < S - 1; ++i)
#pragma unroll 4
    for (int j = i + 1; j < S; ++j) lnL += L.T[i * S + j];
#pragma unroll 4
  for (int i = 0; i < S; ++i) lnL += L.T[i * S + i];
  return lnL;
}

// grid (n, taxa of the band), one wave per pair (j, k), k > j
template <int S> __global__ __launch_bounds__(64) void dist_opt_kernel(const DistPairParams q)
{
  __shared__ DistLds<S> L;
  const int j = q.j0 + (int)blockIdx.y, k = (int)blockIdx.x, lane = threadIdx.x;
  if (k <= j || k >= q.n) return; // (the whole workgroup)
  const long long pair = dist_pair_index(q.n, j, k);
  const double   *g = q.G + (size_t)(j - q.j0) * S * q.ldg + (size_t)k * S;
  const double    len = q.sums[3 * pair];
  for (int x = lane; x < S * S; x += 64)
  {
    const double v = g[(size_t)(x / S) * q.ldg + (x % S)];
    const double f = len > 0.0 ? v / len : v; // src/lk.c:1863-1866
    L.F[x] = f;
    if (q.counts) q.counts[(size_t)(pair - q.pair0) * S * S + x] = f;
    L.U[x] = q.U[x];
    L.V[x] = q.V[x];
  }
  if (lane < S)
  {
    L.pi[lane] = q.pi[lane];
    L.R[lane]  = q.R[lane];
  }
  __syncthreads();
  double sum = 0.0;
  for (int x = 0; x < S * S; ++x) sum += L.F[x]; // :1868-1869
  double init = q.init[pair];
  if (init > kDistMax - kSmall || init < 0.0) init = 0.1; // :1845
  double d_max = init, lnl = 0.0;
  int    iters = 0;
  if (!(sum < .001))
  { // Opt_Dist_F, src/optimiz.c:1958-1972, and Dist_F_Brent, :1848-1953
    const double mdl = q.min_diff_lk, tol = 1.E-10, cgold = 0.3819660, zeps = 1.e-10;
    const int    n_iter_max = 1000;
    const double ax = q.l_min, bx = init < q.l_min ? q.l_min : init, cx = q.l_max;
    double a, b, d = 0.0, etemp, fu, fv, fw, fx, p, qq, r, tol1, tol2, u, v, w, x, xm, e = 0.0;
    double old_lnL, init_lnL, curr_lnL;
    a = ax < cx ? ax : cx;
    b = ax > cx ? ax : cx;
    x = w = v = bx;
    old_lnL = -1.e20; // UNLIKELY
    fu = fv = fw = fx = curr_lnL = init_lnL = u = 0.0;
    // (one call site of Lk_Dist: the evaluation in front of the loop, the one per iteration and the one at the return take turns)
    double arg = fabs(bx);
    int    phase = 0, iter = 0;
    for (;;)
    {
      const double f = dist_lk<S>(L, arg, q.l_min, q.l_max, lane);
      if (phase == 2)
      {
        lnl = f;
        break;
      }
      if (phase == 0)
      {
        fw = fv = fx = -f;
        curr_lnL = init_lnL = -fw;
        phase = 1;
      }
      else
      {
        fu       = -f;
        curr_lnL = -fu;
        if (fu < fx)
        {
          if (u >= x) a = x;
          else b = x;
          v = w; w = x; x = u;
          fv = fw; fw = fx; fx = fu;
        }
        else
        {
          if (u < x) a = u;
          else b = u;
          if (fu < fw || fabs(w - x) < kSmall)
          {
            v = w; w = u;
            fv = fw; fw = fu;
          }
          else if (fu < fv || fabs(v - x) < kSmall || fabs(v - w) < kSmall)
          {
            v = u;
            fv = fu;
          }
        }
      }
      ++iter; // for(iter=1;iter<=BRENT_IT_MAX;iter++)
      xm   = 0.5 * (a + b);
      tol1 = tol * fabs(x) + zeps;
      tol2 = 2.0 * tol1;
      if ((fabs(curr_lnL - old_lnL) < mdl && curr_lnL > init_lnL - mdl) || iter > n_iter_max - 1)
      {
        d_max = x;
        arg   = x;
        iters = iter;
        phase = 2;
        continue;
      }
      if (fabs(e) > tol1)
      {
        r  = (x - w) * (fx - fv);
        qq = (x - v) * (fx - fw);
        p  = (x - v) * qq - (x - w) * r;
        qq = 2.0 * (qq - r);
        if (qq > 0.0) p = -p;
        qq    = fabs(qq);
        etemp = e;
        e     = d;
        if (fabs(p) >= fabs(0.5 * qq * etemp) || p <= qq * (a - x) || p >= qq * (b - x))
        {
          e = x >= xm ? a - x : b - x;
          d = cgold * e;
        }
        else
        {
          d = p / qq;
          u = x + d;
          if (u - a < tol2 || b - u < tol2) d = (xm - x) > 0.0 ? fabs(tol1) : -fabs(tol1); // SIGN(tol1, xm - x)
        }
      }
      else
      {
        e = x >= xm ? a - x : b - x;
        d = cgold * e;
      }
      u       = fabs(d) >= tol1 ? x + d : x + (d > 0.0 ? fabs(tol1) : -fabs(tol1));
      old_lnL = curr_lnL;
      arg     = fabs(u);
    }
  }
  if (d_max >= kDistMax) d_max = kDistMax; // src/lk.c:1883
  if (lane == 0)
  {
    q.dist[pair]  = d_max;
    q.lnl[pair]   = lnl;
    q.iters[pair] = iters;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// K80_dist(data, 1e6) / JC69_Dist of one pair from its sums (src/utilities.c:2470-2503, 2558-2581), with the host's libm
static double dist_start_value(int S, const double *s)
{
  const double len = s[0];
  double       d;
  if (S == 4)
  {
    const double g_shape = 1.E+6;
    double       P = .5, Q = .5;
    if (len > .0)
    {
      P = s[1] / len;
      Q = s[2] / len;
    }
    if ((1 - 2 * P - Q <= .0) || (1 - 2 * Q <= .0)) return -1.;
    d = (g_shape / 2) * (pow(1 - 2 * P - Q, -1. / g_shape) + 0.5 * pow(1 - 2 * Q, -1. / g_shape) - 1.5);
  }
  else
  {
    const double ns = (double)S;
    const double P = len > .0 ? s[1] / len : 1.;
    if ((1. - (ns) / (ns - 1.) * P) < .0) return -1.;
    d = -(ns - 1.) / (ns)*log(1. - (ns) / (ns - 1.) * P);
  }
  if (d > kDistMax) d = kDistMax;
  return d;
}

struct DistOut
{
  const double *in_init;
  double       *dist, *init, *counts, *lnl;
  int          *iters;
};

// sh: the plain instance, or the shards of a one-process sharded instance in pattern order
static int dist_calc(const std::vector<Instance *> &sh, double min_diff_lk, const DistOut &o)
{
  static const char *const who = "phyhip_calculate_pairwise_ml_distances";
  Instance *const I = sh[0];
  auto           &U = side_of(I).dist;
  const int       n = I->tips, S = I->S;
  const size_t nn = (size_t)n * n, np = (size_t)n * (n - 1) / 2, SS = (size_t)S * S;
  for (size_t i = 0; i < nn; ++i) o.dist[i] = 0.0;
  if (o.init)
    for (size_t i = 0; i < nn; ++i) o.init[i] = 0.0;
  if (n < 2) return PHYHIP_SUCCESS;

  // bands of taxa
  const int    ldg = (n * S + 63) / 64 * 64;
  const size_t per_taxon = (size_t)S * ldg * sizeof(double);
  int          band = U.band_bytes / per_taxon > (size_t)n ? n : (int)(U.band_bytes / per_taxon);
  if (band < 1) band = 1;
  if (band > n - 1) band = n - 1;
  const int    nbands = (n - 1 + band - 1) / band;
  const size_t g_rows = ((size_t)band * S + 15) / 16 * 16 + 16, g_elems = g_rows * ldg; // (+16: a band's first row need not start a block)
  bool         other_dev = false;
  for (Instance *X : sh) other_dev = other_dev || X->dev != I->dev;
  const size_t band_pairs = (size_t)band * (n - 1);
  // first shard: counts | a second band (shards on other devices) | sums | init | dist | lnl | iters | normalised counts of a band
  const size_t off_tmp = g_elems, off_sums = off_tmp + (other_dev ? g_elems : 0), off_init = off_sums + 3 * np, off_dist = off_init + np,
               off_lnl = off_dist + np, off_it = off_lnl + np, off_cnt = off_it + (np + 1) / 2, total = off_cnt + (o.counts ? band_pairs * SS : 0);
  int rc;
  if ((rc = make_current(I->dev))) return rc;
  if ((rc = U.work.reserve(total * sizeof(double), who))) return rc;
  if ((rc = upload_masks(I))) return rc;
  for (size_t g = 1; g < sh.size(); ++g)
  {
    if ((rc = make_current(sh[g]->dev))) return rc;
    if ((rc = side_of(sh[g]).dist.work.reserve(g_elems * sizeof(double), who))) return rc;
    if ((rc = upload_masks(sh[g]))) return rc;
  }
  if ((rc = make_current(I->dev))) return rc;
  double *const W = (double *)U.work.ptr;
  double *const d_G = W, *const d_tmp = W + off_tmp, *const d_sums = W + off_sums, *const d_init = W + off_init, *const d_dist = W + off_dist,
               *const d_lnl = W + off_lnl, *const d_cnt = o.counts ? W + off_cnt : nullptr;
  int *const    d_it = (int *)(W + off_it);

  SideTimer tm(I);

  DistPairParams q;
  memset(&q, 0, sizeof q);
  q.G = d_G; q.sums = d_sums; q.init = d_init; q.dist = d_dist; q.lnl = d_lnl; q.counts = d_cnt; q.iters = d_it;
  q.U = I->d_evec; q.V = I->d_ivec; q.R = I->d_eval; q.pi = I->d_pi;
  q.l_min = I->l_min; q.l_max = I->l_max; q.min_diff_lk = min_diff_lk; q.n = n; q.ldg = ldg;

  // the raw counts of the band [j0, j1) on the first shard's device, then the sums of its pairs
  auto count_band = [&](int j0, int j1) -> int {
    const int  rows = (j1 - j0) * S, row_blocks = (rows + 15) / 16;
    const dim3 grid((unsigned)(ldg / 64), (unsigned)row_blocks), block(64);
    int        r2;
    if ((r2 = tm.tic())) return r2;
    for (size_t g = 0; g < sh.size(); ++g)
    {
      Instance *X = sh[g];
      if ((r2 = make_current(X->dev))) return r2;
      DistCountParams c;
      c.tip_codes = X->d_tipcodes; c.code_masks = X->d_masks; c.wght = X->d_wght; c.G = (double *)side_of(X).dist.work.ptr;
      c.P = X->P; c.Ppad = X->Ppad; c.n = n; c.row0 = j0 * S; c.ldg = ldg;
      HIPCHK(hipMemsetAsync(c.G, 0, (size_t)row_blocks * 16 * ldg * sizeof(double), X->stream));
      if (S == 4) hipLaunchKernelGGL(dist_count_kernel<4>, grid, block, 0, X->stream, c);
      else hipLaunchKernelGGL(dist_count_kernel<20>, grid, block, 0, X->stream, c);
      HIPCHK(hipGetLastError());
    }
    if ((r2 = make_current(I->dev))) return r2;
    const size_t used = (size_t)row_blocks * 16 * ldg;
    for (size_t g = 1; g < sh.size(); ++g)
    { // in shard order, on the first shard's device
      Instance *X = sh[g];
      if (X->stream != I->stream) HIPCHK(hipStreamSynchronize(X->stream));
      const double *src = (const double *)side_of(X).dist.work.ptr;
      if (X->dev != I->dev)
      {
        HIPCHK(hipStreamSynchronize(I->stream));
        HIPCHK(hipMemcpyPeer(d_tmp, I->dev, src, X->dev, used * sizeof(double)));
        HIPCHK(hipDeviceSynchronize());
        src = d_tmp;
      }
      hipLaunchKernelGGL(dist_add_kernel, dim3((unsigned)((used + 255) / 256)), dim3(256), 0, I->stream, d_G, src, used);
      HIPCHK(hipGetLastError());
      if (X->stream != I->stream) HIPCHK(hipStreamSynchronize(I->stream)); // (the shard's next band overwrites what was just read)
    }
    DistPairParams s = q;
    s.j0 = j0; s.j1 = j1; s.pair0 = (long long)j0 * n - (long long)j0 * (j0 + 1) / 2;
    const dim3 sgrid((unsigned)((n + 255) / 256), (unsigned)(j1 - j0));
    if (S == 4) hipLaunchKernelGGL(dist_sums_kernel<4>, sgrid, dim3(256), 0, I->stream, s);
    else hipLaunchKernelGGL(dist_sums_kernel<20>, sgrid, dim3(256), 0, I->stream, s);
    HIPCHK(hipGetLastError());
    return tm.toc(U.prof_count_ms);
  };

  std::vector<double> h_init(np), h_sums;
  // the caller's starting values, or K80 / JC69 from the sums with the host's libm
  auto start_values = [&]() -> int {
    if (o.in_init)
    {
      size_t x = 0;
      for (int j = 0; j < n - 1; ++j)
        for (int k = j + 1; k < n; ++k) h_init[x++] = o.in_init[(size_t)j * n + k];
    }
    else
    {
      h_sums.resize(3 * np);
      HIPCHK(hipMemcpyAsync(h_sums.data(), d_sums, 3 * np * sizeof(double), hipMemcpyDeviceToHost, I->stream));
      HIPCHK(hipStreamSynchronize(I->stream));
      for (size_t x = 0; x < np; ++x) h_init[x] = dist_start_value(S, h_sums.data() + 3 * x);
    }
    HIPCHK(hipMemcpyAsync(d_init, h_init.data(), np * sizeof(double), hipMemcpyHostToDevice, I->stream));
    HIPCHK(hipStreamSynchronize(I->stream));
    return 0;
  };

  const bool two_passes = !o.in_init && nbands > 1; // the sums of every band first (a recount is cheaper than keeping all counts)
  if (two_passes)
    for (int j0 = 0; j0 < n - 1; j0 += band)
      if ((rc = count_band(j0, j0 + band < n - 1 ? j0 + band : n - 1))) return rc;
  if (o.in_init || two_passes)
    if ((rc = start_values())) return rc;
  for (int j0 = 0; j0 < n - 1; j0 += band)
  {
    const int j1 = j0 + band < n - 1 ? j0 + band : n - 1;
    if ((rc = count_band(j0, j1))) return rc;
    if (!o.in_init && !two_passes)
      if ((rc = start_values())) return rc;
    DistPairParams s = q;
    s.j0 = j0; s.j1 = j1; s.pair0 = (long long)j0 * n - (long long)j0 * (j0 + 1) / 2;
    if ((rc = tm.tic())) return rc;
    const dim3 ogrid((unsigned)n, (unsigned)(j1 - j0));
    if (S == 4) hipLaunchKernelGGL(dist_opt_kernel<4>, ogrid, dim3(64), 0, I->stream, s);
    else hipLaunchKernelGGL(dist_opt_kernel<20>, ogrid, dim3(64), 0, I->stream, s);
    HIPCHK(hipGetLastError());
    if ((rc = tm.toc(U.prof_opt_ms))) return rc;
    if (o.counts)
    {
      const long long p1 = (long long)j1 * n - (long long)j1 * (j1 + 1) / 2;
      HIPCHK(hipMemcpyAsync(o.counts + (size_t)s.pair0 * SS, d_cnt, (size_t)(p1 - s.pair0) * SS * sizeof(double), hipMemcpyDeviceToHost, I->stream));
      HIPCHK(hipStreamSynchronize(I->stream));
    }
  }
  std::vector<double> h_dist(np), h_lnl(o.lnl ? np : 0);
  HIPCHK(hipMemcpyAsync(h_dist.data(), d_dist, np * sizeof(double), hipMemcpyDeviceToHost, I->stream));
  if (o.lnl) HIPCHK(hipMemcpyAsync(o.lnl, d_lnl, np * sizeof(double), hipMemcpyDeviceToHost, I->stream));
  if (o.iters) HIPCHK(hipMemcpyAsync(o.iters, d_it, np * sizeof(int), hipMemcpyDeviceToHost, I->stream));
  HIPCHK(hipStreamSynchronize(I->stream));
  if (I->prof) ++U.prof_n;
  size_t x = 0;
  for (int j = 0; j < n - 1; ++j)
    for (int k = j + 1; k < n; ++k, ++x)
    {
      o.dist[(size_t)j * n + k] = o.dist[(size_t)k * n + j] = h_dist[x];
      if (o.init) o.init[(size_t)j * n + k] = o.init[(size_t)k * n + j] = h_init[x];
    }
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

int phyhip_calculate_pairwise_ml_distances(int instance, int eigenIndex, int stateFrequenciesIndex, double minDiffLk,
                                           const double *inInitialDistances, double *outDistances, double *outInitialDistances,
                                           double *outCounts, double *outLogLikelihoods, int *outIterations)
{
  if (!outDistances) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_calculate_pairwise_ml_distances: outDistances is NULL");
  static const char *const who = "phyhip_calculate_pairwise_ml_distances";
  SideShards s;
  // (the refusals that belong to the kind of instance come before the ones about this call's arguments)
  int rc = side_collect(instance, who, kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop, s);
  if (rc < 0) return rc;
  const std::vector<Instance *> &sh = s.sh;
  if ((rc = refuse_kind(sh[0], who, kRefuseStates))) return rc;
  if (!(minDiffLk > 0.0)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "minDiffLk %g (must be > 0)", minDiffLk);
  if (eigenIndex < 0 || eigenIndex >= sh[0]->NE) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "eigenIndex %d (0..%d)", eigenIndex, sh[0]->NE - 1);
  if (stateFrequenciesIndex < 0 || stateFrequenciesIndex >= sh[0]->NE)
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "stateFrequenciesIndex %d (0..%d)", stateFrequenciesIndex, sh[0]->NE - 1);
  return dist_calc(sh, minDiffLk, DistOut{inInitialDistances, outDistances, outInitialDistances, outCounts, outLogLikelihoods, outIterations});
}

int phyhip_set_pairwise_work_space(int instance, long long maxBytes)
{
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    side_of(I).dist.band_bytes = maxBytes > 0 ? (size_t)maxBytes : kDistBandBytes;
    return 0;
  });
}

int phyhip_profile_read_pairwise(int instance, double *outCountMs, double *outOptimiseMs, int *outCalls)
{
  double a = 0.0, b = 0.0;
  int    n = 0;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).dist;
    a += U.prof_count_ms;
    b += U.prof_opt_ms;
    n += U.prof_n;
    U.prof_count_ms = U.prof_opt_ms = 0.0;
    U.prof_n = 0;
    return 0;
  });
  if (rc < 0) return rc;
  if (outCountMs) *outCountMs = a;
  if (outOptimiseMs) *outOptimiseMs = b;
  if (outCalls) *outCalls = n;
  return PHYHIP_SUCCESS;
}

} // extern "C"
