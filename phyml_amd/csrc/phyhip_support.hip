// phyhip_support.hip -- the resampling behind SH-like branch supports: phyhip_set_support_site_log_likelihoods,
// phyhip_calculate_sh_support, phyhip_get_support_alias_table (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// aLRT() (src/alrt.c:172-226) stores c_lnL_sorted of the three NNI configurations of an internal edge in log_lks_aLRT[0..2], then
// Statistics_To_SH (src/alrt.c:1148-1298) draws 10 000 replicates of init_len sites each with Sample_n_i_With_Proba_pi
// (src/stats.c:4493-4578: an alias table over the pattern weights), sums the three vectors over the drawn patterns, centres the sums
// on the totals and counts delta > delta_local + 0.1.  10 000 x init_len draws per internal edge, on one host thread.  Here:
//   * the three vectors live in device slots (3 x P doubles on the first shard's device), filled by an upload or -- NULL -- by a
//     device-to-device copy of what the last edge evaluation left (log_lks_aLRT[k][site] = c_lnL_sorted[site], no download);
//   * the alias table is Sample_n_i_With_Proba_pi's construction, operation for operation, in plain sequential C on the host side
//     (support_build_alias), once per weight vector and site count;
//   * support_table_kernel writes one 64-byte row per pattern, {prob, l0 l1 l2 of the column, l0 l1 l2 of its alias, 0}: a draw is
//     ONE gather with no dependent second load;
//   * support_totals_kernel: c_k = sum over the patterns in ascending order of log_lks[k][p] * w[p], one lane per k (src/alrt.c:1172-1177);
//   * support_draw_kernel: one wave per replicate, grid-strided over the replicates.  Lane l takes the draw pairs l, l + 64, ..; pair
//     j of replicate r is ONE Philox4x32-10 block, counter (j, 0, r, 0), key (seed low word, seed high word): draw 2j from words
//     (w0, w1), draw 2j+1 from (w2, w3).  column = (w_a * P) >> 32 (never P); the draw keeps the column if w_b * 2^-32 < prob[column],
//     else takes its alias.  Each lane adds its draws in ascending order into three FP64 partial sums; the 64 partial sums meet in a
//     fixed butterfly (lane distance 32, 16, .., 1): no floating-point atomics, and -- a replicate being one wave whatever the grid --
//     the same bits from run to run, for any grid and any replicate count.  Lane 0 centres, restates the two six-way orderings of
//     src/alrt.c:1184-1216 / 1254-1287 line by line (ties included), and stores the two 0/1 flags of the replicate;
//   * support_count_kernel adds the flags (integers).
// The call writes a work space of its own: partials, scale vectors, matrices, the last evaluation's outputs and the numerical
// warning stay what they were.
#include "phyhip_side.hpp"

namespace phyhip_host
{

constexpr int kSupRow = 8;          // doubles per row of the gather table (64 bytes)
constexpr int kSupWavesPerWg = 4;   // replicates in flight per workgroup of support_draw_kernel

// ---- Philox4x32-10 (Salmon et al., SC'11): counter-based, integers only ------------------------------------------------------------
struct Philox4
{
  uint32_t w[4];
};
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
  for (int round = 0; round < 10; ++round)
  {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

struct SupportParams
{
  const double *slots;  // [3][P]
  const double *wght;   // [P] (all shards, global order)
  const double *prob;   // [P]
  const int    *alias;  // [P]
  double       *table;  // [P][kSupRow]
  double       *totals; // [3]
  double       *sums;   // [replicates][3], the uncentred sums
  int          *flags;  // [2][replicates]: accepted, RELL
  int          *counts; // [2]
  long long     P;
  int           sites, replicates;
  uint32_t      key0, key1;
};

__global__ __launch_bounds__(256) void support_table_kernel(const SupportParams q)
{
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= q.P) return;
  const long long a = q.alias[p];
  double         *row = q.table + (size_t)p * kSupRow;
  row[0] = q.prob[p];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    row[1 + k] = q.slots[(size_t)k * q.P + p];
    row[4 + k] = q.slots[(size_t)k * q.P + a];
  }
  row[7] = 0.0;
}

// one wave; lane k < 3 forms c_k in the reference's order (the rounded product, then the addition).  The additions are a dependent
// chain by construction; the loads and the products are not: eight patterns' worth are formed ahead of the eight additions
__global__ __launch_bounds__(64) void support_totals_kernel(const SupportParams q)
{
  const int k = threadIdx.x;
  if (k >= 3) return;
  const double *l = q.slots + (size_t)k * q.P;
  double        c = 0.0;
  long long     p = 0;
  for (; p + 8 <= q.P; p += 8)
  {
    double t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = l[p + i] * q.wght[p + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) c += t[i];
  }
  for (; p < q.P; ++p) c += l[p] * q.wght[p];
  q.totals[k] = c;
}

__device__ __forceinline__ void support_one_draw(const SupportParams &q, uint32_t wa, uint32_t wb, double &s0, double &s1, double &s2)
{
  const uint32_t column = (uint32_t)(((unsigned long long)wa * (unsigned long long)q.P) >> 32);
  const double2 *row = reinterpret_cast<const double2 *>(q.table + (size_t)column * kSupRow);
  const double2  a = row[0], b = row[1], c = row[2], d = row[3]; // {prob, l0} {l1, l2} {a0, a1} {a2, 0}
  const bool     keep = (double)wb * 0x1p-32 < a.x;
  s0 += keep ? a.y : c.x;
  s1 += keep ? b.x : c.y;
  s2 += keep ? b.y : d.x;
}

// the six-way ordering of src/alrt.c:1184-1216 (and :1254-1287): the gap between the largest and the second largest
__host__ __device__ __forceinline__ double support_delta(double c0, double c1, double c2)
{
  double delta;
  if (c0 >= c1 && c0 >= c2)
  {
    if (c1 >= c2) delta = c0 - c1;
    else delta = c0 - c2;
  }
  else if (c1 >= c0 && c1 >= c2)
  {
    if (c0 >= c2) delta = c1 - c0;
    else delta = c1 - c2;
  }
  else
  {
    if (c1 >= c0) delta = c2 - c1;
    else delta = c2 - c0;
  }
  return delta;
}

// grid: any; workgroup: kSupWavesPerWg waves, a replicate per wave
__global__ __launch_bounds__(64 * kSupWavesPerWg) void support_draw_kernel(const SupportParams q)
{
  const int lane = threadIdx.x & 63;
  const int wave = (int)blockIdx.x * kSupWavesPerWg + ((int)threadIdx.x >> 6), nwaves = (int)gridDim.x * kSupWavesPerWg;
  const int pairs = q.sites >> 1; // whole pairs; an odd site count leaves one more draw, the first of pair `pairs`
  const double c0 = q.totals[0], c1 = q.totals[1], c2 = q.totals[2];
  const double delta = support_delta(c0, c1, c2);
  for (int r = wave; r < q.replicates; r += nwaves)
  {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 2
    for (int j = lane; j < pairs; j += 64)
    {
      const Philox4 x = philox4x32_10((uint32_t)j, 0u, (uint32_t)r, 0u, q.key0, q.key1);
      support_one_draw(q, x.w[0], x.w[1], s0, s1, s2);
      support_one_draw(q, x.w[2], x.w[3], s0, s1, s2);
    }
    if ((q.sites & 1) && (pairs & 63) == lane)
    { // (the lane whose turn pair `pairs` is: its second draw is dropped)
      const Philox4 x = philox4x32_10((uint32_t)pairs, 0u, (uint32_t)r, 0u, q.key0, q.key1);
      support_one_draw(q, x.w[0], x.w[1], s0, s1, s2);
    }
    // the 64 partial sums in a fixed butterfly: every lane ends with the same three doubles
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
      s0 += __shfl_xor(s0, off, 64);
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    if (lane == 0)
    {
      if (q.sums)
      {
        q.sums[(size_t)r * 3 + 0] = s0;
        q.sums[(size_t)r * 3 + 1] = s1;
        q.sums[(size_t)r * 3 + 2] = s2;
      }
      const int rell = (s0 >= s1 && s0 >= s2) ? 1 : 0;                // src/alrt.c:1129, on the uncentred sums
      const double lk0 = s0 - c0, lk1 = s1 - c1, lk2 = s2 - c2;       // :1249-1251
      const double delta_local = support_delta(lk0, lk1, lk2);        // :1254-1287
      q.flags[r] = delta > (delta_local + 0.1) ? 1 : 0;               // :1289
      q.flags[(size_t)q.replicates + r] = rell;
    }
  }
}

// one workgroup: counts[0] = accepted replicates, counts[1] = RELL replicates
__global__ __launch_bounds__(256) void support_count_kernel(const SupportParams q)
{
  __shared__ int part[2][4];
  int            a = 0, b = 0;
  for (int r = threadIdx.x; r < q.replicates; r += 256)
  {
    a += q.flags[r];
    b += q.flags[(size_t)q.replicates + r];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if ((threadIdx.x & 63) == 0)
  {
    part[0][threadIdx.x >> 6] = a;
    part[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    q.counts[0] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    q.counts[1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// Sample_n_i_With_Proba_pi's table (src/stats.c:4493-4560), operation for operation: pi = w / init_len, sum, p = pi * len / sum, the
// descending fill of small / large, the pairing loop, the leftovers set to 1 (their alias stays 0, as calloc leaves it).
// 0, or -1 for a negative weight, -2 where the sum is 0 (the reference exits at both).
static int support_build_alias(const std::vector<double> &w, int init_len, std::vector<double> &prob, std::vector<int> &alias)
{
  const int           len = (int)w.size();
  std::vector<double> pi(len), p(len);
  std::vector<int>    small(len), large(len);
  int                 num_small = 0, num_large = 0, a, g, i;
  prob.assign(len, 0.0);
  alias.assign(len, 0);
  for (i = 0; i < len; ++i) pi[i] = w[i] / (double)init_len; // src/alrt.c:1229
  double sum = .0;
  for (i = 0; i < len; i++)
  {
    if (pi[i] < 0) return -1;
    sum += pi[i];
  }
  if (sum == 0.) return -2;
  for (i = 0; i < len; i++) p[i] = pi[i] * len / sum;
  for (i = len - 1; i >= 0; --i)
  {
    if (p[i] < 1) small[num_small++] = i;
    else large[num_large++] = i;
  }
  while (num_small && num_large)
  {
    a        = small[--num_small];
    g        = large[--num_large];
    prob[a]  = p[a];
    alias[a] = g;
    p[g]     = p[g] + p[a] - 1;
    if (p[g] < 1) small[num_small++] = g;
    else large[num_large++] = g;
  }
  while (num_large) prob[large[--num_large]] = 1;
  while (num_small) prob[small[--num_small]] = 1;
  return 0;
}

// the alias table of the instance's weights and `sites`, built on the host once per weight vector and site count (SideUnits::sup)
static int support_alias(const SideShards &s, int sites, const char *who)
{
  const std::vector<Instance *> &sh = s.sh;
  const long long                P = s.P;
  Instance *const    I = sh[0];
  auto              &U = side_of(I).sup;
  unsigned long long epoch = 0;
  for (Instance *X : sh) epoch += X->wght_epoch; // (each only ever grows)
  if (U.alias_valid && U.epoch == epoch && U.sites == sites && (long long)U.w.size() == P) return 0;
  U.alias_valid = U.table_on_device = false;
  U.w.resize((size_t)P);
  for (size_t g = 0; g < sh.size(); ++g)
  { // (weights are set synchronously: nothing queued can change them)
    int rc;
    if ((rc = make_current(sh[g]->dev))) return rc;
    HIPCHK(hipMemcpy(U.w.data() + s.lo[g], sh[g]->d_wght, (size_t)sh[g]->P * sizeof(double), hipMemcpyDeviceToHost));
  }
  const int rc = support_build_alias(U.w, sites, U.prob, U.alias);
  if (rc == -1) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: a negative pattern weight", who);
  if (rc == -2) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: every pattern weight is zero", who);
  U.epoch = epoch;
  U.sites = sites;
  U.alias_valid = true;
  return make_current(I->dev);
}

struct SupportOut
{
  double *sh, *rell, *totals, *sums;
  int    *accepted;
};

static int support_calc(const SideShards &s, int sites, int replicates, unsigned long long seed, const SupportOut &o)
{
  static const char *const who = "phyhip_calculate_sh_support";
  Instance *const          I = s.sh[0];
  auto                    &U = side_of(I).sup;
  const long long          P = s.P;
  int                      rc;
  if ((rc = support_alias(s, sites, who))) return rc;
  if ((rc = make_current(I->dev))) return rc;
  // work space: weights | prob | table (its 64-byte rows on 64-byte boundaries) | totals (4) | alias (ints) -- what depends on the
  // patterns alone, so that it stays where it was uploaded whatever the replicate count of the next call -- then sums | flags, counts (ints)
  const size_t uP = (size_t)P, R = (size_t)replicates;
  const size_t off_prob = uP, off_table = (off_prob + uP + kSupRow - 1) / kSupRow * kSupRow, off_tot = off_table + uP * kSupRow, off_alias = off_tot + 4, off_sums = off_alias + (uP + 1) / 2,
               off_int = off_sums + 3 * R;
  const size_t n_int = 2 * R + 2, total = (off_int + (n_int + 1) / 2) * sizeof(double);
  if (!U.work.holds(total))
  { // (what is still running reads the memory about to be freed; the uploaded table goes with it)
    HIPCHK(hipStreamSynchronize(I->stream));
    U.table_on_device = false;
    if ((rc = U.work.reserve(total, who))) return rc;
  }
  double *const W = (double *)U.work.ptr;
  int *const    d_alias = (int *)(W + off_alias), *const Wi = (int *)(W + off_int);
  SupportParams q;
  memset(&q, 0, sizeof q);
  q.slots = (const double *)U.slots.ptr; q.wght = W; q.prob = W + off_prob; q.alias = d_alias; q.table = W + off_table; q.totals = W + off_tot;
  q.sums = o.sums ? W + off_sums : nullptr; q.flags = Wi; q.counts = Wi + 2 * R;
  q.P = P; q.sites = sites; q.replicates = replicates;
  q.key0 = (uint32_t)seed; q.key1 = (uint32_t)(seed >> 32);
  if (!U.table_on_device || U.dev_P != P)
  { // (pageable memory: the copies have left the host vectors when the calls return)
    HIPCHK(hipMemcpyAsync(W, U.w.data(), uP * sizeof(double), hipMemcpyHostToDevice, I->stream));
    HIPCHK(hipMemcpyAsync(W + off_prob, U.prob.data(), uP * sizeof(double), hipMemcpyHostToDevice, I->stream));
    HIPCHK(hipMemcpyAsync(d_alias, U.alias.data(), uP * sizeof(int), hipMemcpyHostToDevice, I->stream));
    HIPCHK(hipStreamSynchronize(I->stream));
    U.table_on_device = true;
    U.dev_P = P;
  }
  SideTimer tm(I);
  if ((rc = tm.tic())) return rc;
  hipLaunchKernelGGL(support_table_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, I->stream, q);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(support_totals_kernel, dim3(1), dim3(64), 0, I->stream, q);
  HIPCHK(hipGetLastError());
  const int want = (replicates + kSupWavesPerWg - 1) / kSupWavesPerWg, cap = (I->cus > 0 ? I->cus : 256) * 8;
  hipLaunchKernelGGL(support_draw_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * kSupWavesPerWg), 0, I->stream, q);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(support_count_kernel, dim3(1), dim3(256), 0, I->stream, q);
  HIPCHK(hipGetLastError());
  if ((rc = tm.mark())) return rc;
  int    counts[2] = {0, 0};
  double totals[3];
  HIPCHK(hipMemcpyAsync(counts, q.counts, sizeof counts, hipMemcpyDeviceToHost, I->stream));
  HIPCHK(hipMemcpyAsync(totals, q.totals, sizeof totals, hipMemcpyDeviceToHost, I->stream));
  if (o.sums) HIPCHK(hipMemcpyAsync(o.sums, q.sums, 3 * R * sizeof(double), hipMemcpyDeviceToHost, I->stream));
  if (o.accepted) HIPCHK(hipMemcpyAsync(o.accepted, q.flags, R * sizeof(int), hipMemcpyDeviceToHost, I->stream));
  HIPCHK(hipStreamSynchronize(I->stream));
  if ((rc = tm.toc(U.prof_ms))) return rc;
  if (I->prof) ++U.prof_n;
  if (o.sh) *o.sh = (double)counts[0] / (double)replicates;     // res = nb / occurence
  if (o.rell) *o.rell = (double)counts[1] / (double)replicates;
  if (o.totals)
    for (int k = 0; k < 3; ++k) o.totals[k] = totals[k];
  return PHYHIP_SUCCESS;
}

static int support_set_slot(const SideShards &s, int slot, const double *in)
{
  static const char *const who = "phyhip_set_support_site_log_likelihoods";
  const std::vector<Instance *> &sh = s.sh;
  const std::vector<long long>  &lo = s.lo;
  const long long          P = s.P;
  Instance *const          I = sh[0];
  auto                    &U = side_of(I).sup;
  int                      rc;
  if (in == nullptr)
    for (Instance *X : sh)
    { // as phyhip_get_site_log_likelihoods: what is queued runs first
      if ((rc = make_current(X->dev))) return rc;
      if ((rc = flush_sync(X))) return rc;
    }
  if ((rc = make_current(I->dev))) return rc;
  if (!U.slots.ptr)
  {
    if ((rc = U.slots.reserve(3 * (size_t)P * sizeof(double), who))) return rc;
    U.slot_set[0] = U.slot_set[1] = U.slot_set[2] = false;
  }
  double *const dst = (double *)U.slots.ptr + (size_t)slot * (size_t)P;
  HIPCHK(hipStreamSynchronize(I->stream)); // (a resampling still reading the slot)
  if (in)
  {
    HIPCHK(hipMemcpy(dst, in, (size_t)P * sizeof(double), hipMemcpyHostToDevice));
  }
  else
    for (size_t g = 0; g < sh.size(); ++g)
    {
      Instance *X = sh[g];
      const size_t bytes = (size_t)X->P * sizeof(double);
      if (X->dev == I->dev) HIPCHK(hipMemcpy(dst + lo[g], X->d_site_lnl, bytes, hipMemcpyDeviceToDevice));
      else HIPCHK(hipMemcpyPeer(dst + lo[g], I->dev, X->d_site_lnl, X->dev, bytes));
    }
  U.slot_set[slot] = true;
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

// (every entry point: the plain instance or the shards in pattern order, and the refusals that belong to the kind of instance)
constexpr unsigned kSupportRefuses = kRefuseRank | kRefuseClassAxis | kRefuseGenericLoop;

int phyhip_set_support_site_log_likelihoods(int instance, int slot, const double *inSiteLogLikelihoods)
{
  SideShards s;
  const int  rc = side_collect(instance, "phyhip_set_support_site_log_likelihoods", kSupportRefuses, s);
  if (rc < 0) return rc;
  if (slot < 0 || slot > 2) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_set_support_site_log_likelihoods: slot %d (0..2)", slot);
  return support_set_slot(s, slot, inSiteLogLikelihoods);
}

int phyhip_calculate_sh_support(int instance, int siteCount, int replicateCount, unsigned long long seed, double *outSH, double *outRELL,
                                double *outTotals, double *outReplicateSums, int *outAccepted)
{
  SideShards s;
  const int  rc = side_collect(instance, "phyhip_calculate_sh_support", kSupportRefuses, s);
  if (rc < 0) return rc;
  if (siteCount <= 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_calculate_sh_support: siteCount %d (must be > 0)", siteCount);
  if (replicateCount <= 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_calculate_sh_support: replicateCount %d (must be > 0)", replicateCount);
  const auto &U = side_of(s.sh[0]).sup;
  for (int k = 0; k < 3; ++k)
    if (!U.slots.ptr || !U.slot_set[k])
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_calculate_sh_support: slot %d was never set (phyhip_set_support_site_log_likelihoods)", k);
  return support_calc(s, siteCount, replicateCount, seed, SupportOut{outSH, outRELL, outTotals, outReplicateSums, outAccepted});
}

int phyhip_get_support_alias_table(int instance, int siteCount, double *outProb, int *outAlias)
{
  SideShards s;
  int        rc = side_collect(instance, "phyhip_get_support_alias_table", kSupportRefuses, s);
  if (rc < 0) return rc;
  if (siteCount <= 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_get_support_alias_table: siteCount %d (must be > 0)", siteCount);
  if ((rc = support_alias(s, siteCount, "phyhip_get_support_alias_table"))) return rc;
  const auto &U = side_of(s.sh[0]).sup;
  if (outProb) memcpy(outProb, U.prob.data(), (size_t)s.P * sizeof(double));
  if (outAlias) memcpy(outAlias, U.alias.data(), (size_t)s.P * sizeof(int));
  return PHYHIP_SUCCESS;
}

int phyhip_profile_read_support(int instance, double *outKernelMs, int *outCalls)
{
  double ms = 0.0;
  int    n = 0;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).sup;
    ms += U.prof_ms;
    n += U.prof_n;
    U.prof_ms = 0.0;
    U.prof_n = 0;
    return 0;
  });
  if (rc < 0) return rc;
  if (outKernelMs) *outKernelMs = ms;
  if (outCalls) *outCalls = n;
  return PHYHIP_SUCCESS;
}

} // extern "C"
