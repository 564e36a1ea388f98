// phyhip_pars.hip -- parsimony scores on the device: phyhip_set_parsimony, phyhip_update_partial_parsimony,
// phyhip_calculate_edge_parsimony, phyhip_get_site_parsimony, phyhip_get_partial_parsimony, phyhip_profile_read_parsimony
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// src/pars.c is the second evaluation surface of the tree search: Update_Partial_Pars (src/pars.c:239-393) fills one edge side per
// call from the two sides below it, Pars (src/pars.c:20-52) scores an edge with Pars_Core (src/pars.c:397-437) per pattern and adds
// site_pars * wght.  Two modes, as there:
//   * Fitch (general_pars == NO): per pattern and buffer one int2 {ui, pars}, pattern-contiguous;
//     pars = p1 + p2; ui = u1 & u2; if(!ui){ ++pars; ui = u1 | u2; }          site_pars = pars_l + pars_r + !(ui_l & ui_r)
//   * step matrix (general_pars == YES): int32 [S][Pp] per buffer, pattern fastest;
//     p[i] = min_j(p1[j] + step[i][j]) + min_j(p2[j] + step[i][j])             site_pars = min_i(min_l[i] + min_r[i])
//     in the reference's own int arithmetic, every minimum starting from MAX_PARS as there.  The step matrix is the caller's.
// Buffers share the index space of the partials buffers: k < tipCount is tip k, read from the allowed-state masks the instance
// already holds (Fitch: ui = mask, pars = 0; step matrix: 0 where allowed, MAX_PARS elsewhere -- Init_Ui_Tips / Init_Partial_Pars_Tips,
// src/pars.c:111-235, run the likelihood's own character encoders); k >= tipCount is the plane that goes with partials buffer k.
//
// One launch executes an ordered list of operations (dest, child1, child2) and then, if asked, scores an edge.  A lane owns the same
// patterns for the whole list, so every child written earlier in the launch was written by the lane that reads it: plain loads and
// stores, no grid barrier, nothing between workgroups.  pars_fitch_kernel: two patterns per lane (16-byte loads and stores), the
// operation records at wave-uniform addresses, the children of the NEXT operation loaded before this one's result is stored -- which
// is only right because a child that IS this operation's result is never loaded: the host marks it in the record (bits 0 / 1 of
// `flags`, set whenever the child is the previous record's destination) and the lane takes it from registers.
// The weighted sum is a 64-bit integer: per lane, wave shuffle, one atomic add per wave into a zeroed word -- integer adds commute,
// the result is the same for any grid.  Weights that are not integers are refused (the reference truncates a double into an int at
// every pattern, which is order-dependent: the host layer runs that loop over the downloaded site_pars).
// phyhip_calculate_regraft_parsimony, phyhip_get_regraft_site_parsimony, phyhip_get_regraft_partial_parsimony and
// phyhip_profile_read_regraft_parsimony: K regraft candidates of Spr_Pars in one call (the kernels and their comment: below the step
// matrix; the host driver: phyhip_scan.hpp).
// The queue of this unit is its own: no call here flushes a queued likelihood operation or writes partials, scale vectors,
// matrices, site outputs or the warning flag, and none is a step of the call sequence the resident evaluators watch.
#include "phyhip_scan.hpp"
#include "phyhip_layout.hpp"

namespace phyhip_host
{

constexpr int kParsTile = 256;         // patterns per workgroup of both kernels (phyml_amd/capi.py: PARS_TILE)
constexpr int kParsStaging = 4096;     // operations a launch takes: a longer queue is launched as it fills (capi.py: PARS_STAGING)
constexpr int kMaxPars = 1000000000;   // MAX_PARS, src/utilities.h

struct ParsParams
{
  const uint8_t      *tip_codes;
  const uint32_t     *code_masks;
  int2               *fitch; // [inner buffer][Pp]
  int                *gen;   // [inner buffer][S][Pp]
  const int          *step;  // [S][S], row = parent state
  const int4         *ops;   // {dest, child1, child2, flags}
  int                *site;  // [Pp]
  const long long    *w;     // [Pp] (nullptr: no sum)
  unsigned long long *sum;
  long long           P, Pp, Ppad;
  int                 n_ops, tips, score, b1, b2;
};

struct ParsState
{
  int        general = 0;
  long long  Pp = 0;
  int        ninner = 0;
  int2      *d_fitch = nullptr;
  int       *d_gen = nullptr, *d_step = nullptr, *d_site = nullptr;
  long long *d_w = nullptr;
  unsigned long long *d_sum = nullptr, *h_sum = nullptr;
  int4      *d_ops[2] = {nullptr, nullptr}, *h_ops[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool       ev_pending[2] = {false, false};
  int        slot = 0;
  std::vector<int4> pending;
  int        last_dest = -1;
  unsigned long long w_epoch = ~0ull; // Instance::wght_epoch the integer weights were made from
  bool       w_integer = false;
  bool       scored = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pairs;
  double     prof_ms = 0.0, prof_updates = 0.0;
  int        prof_n = 0;
  struct
  { // phyhip_calculate_regraft_parsimony
    WorkSpace      work;               // as `lay` places it
    ParsScanLayout lay;                // of the last call (phyhip_scan_plan.hpp): the getters read through it
    bool           keep_valid = false; // the last call kept a candidate: the two getters may read it
    std::vector<ParsScanRec>        recs;
    std::vector<unsigned long long> down;
    double         prof_ms = 0.0;      // while profiling: its kernels (phyhip_profile_read_regraft_parsimony)
    int            prof_n = 0;
    long long      prof_cand = 0;      // ... and the candidates they served
  } scan;
};

// ---- Fitch -------------------------------------------------------------------------------------------------------------------------

template <int S> __device__ __forceinline__ int4 fitch_load(const ParsParams &q, int b, long long p, bool two)
{
  if (b < q.tips)
  {
    const uint32_t m0 = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, b, p);
    const uint32_t m1 = two ? tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, b, p + 1) : 0u;
    return make_int4((int)m0, 0, (int)m1, 0);
  }
  return *reinterpret_cast<const int4 *>(q.fitch + (size_t)(b - q.tips) * q.Pp + p);
}

__device__ __forceinline__ int4 fitch_join(const int4 a, const int4 b)
{ // src/pars.c:380-391, two patterns
  int4 r;
  r.y = a.y + b.y;
  r.x = a.x & b.x;
  if (!r.x) { ++r.y; r.x = a.x | b.x; }
  r.w = a.w + b.w;
  r.z = a.z & b.z;
  if (!r.z) { ++r.w; r.z = a.z | b.z; }
  return r;
}

__device__ __forceinline__ void pars_add_sum(const ParsParams &q, long long acc)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0 && acc != 0) atomicAdd(q.sum, (unsigned long long)acc);
}

template <int S> __global__ __launch_bounds__(kParsTile / 2) void pars_fitch_kernel(const ParsParams q)
{
  const long long p = ((long long)blockIdx.x * (kParsTile / 2) + threadIdx.x) * 2; // (p + 1 < Pp: Pp is even)
  const bool      in = p < q.P, two = p + 1 < q.P;
  long long       acc = 0;
  if (in)
  {
    int4 a = make_int4(0, 0, 0, 0), b = a, d = a;
    if (q.n_ops > 0)
    {
      const int4 r = q.ops[0];
      a = fitch_load<S>(q, r.y, p, two);
      b = fitch_load<S>(q, r.z, p, two);
    }
    for (int k = 0; k < q.n_ops; ++k)
    {
      const int4 r = q.ops[k];
      const bool more = k + 1 < q.n_ops;
      int4       nr = make_int4(0, 0, 0, 0), na = nr, nb = nr;
      if (more)
      { // the next operation's children, before this result is stored (a child that is this result is flagged, never loaded)
        nr = q.ops[k + 1];
        if (!(nr.w & 1)) na = fitch_load<S>(q, nr.y, p, two);
        if (!(nr.w & 2)) nb = fitch_load<S>(q, nr.z, p, two);
      }
      d = fitch_join(a, b);
      *reinterpret_cast<int4 *>(q.fitch + (size_t)(r.x - q.tips) * q.Pp + p) = d;
      a = (nr.w & 1) ? d : na;
      b = (nr.w & 2) ? d : nb;
    }
    if (q.score)
    { // src/pars.c:432-433
      const int4 l = fitch_load<S>(q, q.b1, p, two), r = fitch_load<S>(q, q.b2, p, two);
      const int  s0 = l.y + r.y + ((l.x & r.x) ? 0 : 1), s1 = l.w + r.w + ((l.z & r.z) ? 0 : 1);
      q.site[p] = s0;
      if (two) q.site[p + 1] = s1;
      if (q.w) acc = (long long)s0 * q.w[p] + (two ? (long long)s1 * q.w[p + 1] : 0ll);
    }
  }
  if (q.score && q.w) pars_add_sum(q, acc);
}

// ---- step matrix -------------------------------------------------------------------------------------------------------------------

// the S values of buffer b at pattern p into registers (a tip: 0 where the state is allowed, MAX_PARS elsewhere)
template <int S> __device__ __forceinline__ void general_load(const ParsParams &q, int b, long long p, int (&v)[S])
{
  if (b < q.tips)
  {
    const uint32_t mask = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, b, p);
#pragma unroll
    for (int j = 0; j < S; ++j) v[j] = ((mask >> j) & 1u) ? 0 : kMaxPars;
  }
  else
  {
    const int *src = q.gen + (size_t)(b - q.tips) * S * q.Pp + p;
#pragma unroll
    for (int j = 0; j < S; ++j) v[j] = src[(size_t)j * q.Pp];
  }
}

// Per parent state i: min(MAX_PARS, min_j(v1[j] + step[i][j])) + the same of v2 (src/pars.c:359-375, :411-427), stored to dst (an
// operation) or, dst == nullptr, reduced to their minimum (the score).  Both children in registers; row i of the matrix from LDS at a
// wave-uniform address -- the loop over i stays a loop (20 states: unrolled, the 400 matrix entries would be hoisted into registers)
template <int S> __device__ __forceinline__ int general_step(const ParsParams &q, const int *step, int b1, int b2, long long p, int *dst)
{
  int v1[S], v2[S];
  general_load<S>(q, b1, p, v1);
  general_load<S>(q, b2, p, v2);
  int           site = kMaxPars;
  constexpr int kRows = S <= 4 ? S : 1;
#pragma unroll kRows
  for (int i = 0; i < S; ++i)
  {
    int m1 = kMaxPars, m2 = kMaxPars;
#pragma unroll
    for (int j = 0; j < S; ++j)
    {
      const int st = step[i * S + j], x1 = v1[j] + st, x2 = v2[j] + st;
      m1 = x1 < m1 ? x1 : m1;
      m2 = x2 < m2 ? x2 : m2;
    }
    const int t = m1 + m2;
    if (dst) dst[(size_t)i * q.Pp] = t;
    site = t < site ? t : site;
  }
  return site;
}

template <int S> __global__ __launch_bounds__(kParsTile) void pars_general_kernel(const ParsParams q)
{
  __shared__ int step[S * S];
  for (int i = threadIdx.x; i < S * S; i += kParsTile) step[i] = q.step[i];
  __syncthreads();
  const long long p = (long long)blockIdx.x * kParsTile + threadIdx.x;
  const bool      in = p < q.P;
  long long       acc = 0;
  if (in)
  {
    for (int k = 0; k < q.n_ops; ++k)
    {
      const int4 r = q.ops[k];
      general_step<S>(q, step, r.y, r.z, p, q.gen + (size_t)(r.x - q.tips) * S * q.Pp + p);
    }
    if (q.score)
    {
      const int site = general_step<S>(q, step, q.b1, q.b2, p, nullptr);
      q.site[p] = site;
      if (q.w) acc = (long long)site * q.w[p];
    }
  }
  if (q.score && q.w) pars_add_sum(q, acc);
}

// ---- regraft scan ------------------------------------------------------------------------------------------------------------------
// phyhip_calculate_regraft_parsimony: candidate k is J = the join of (child1, child2) -- an Update_Partial_Pars that stores nothing
// -- and the score of the edge (J, subtree).  Grid: x = pattern tiles, y = slabs of the launch's candidates; a workgroup walks its
// slab's records (wave-uniform addresses), the next record's operands loaded before this candidate is reduced.  Bit 0 of a record's
// flags: its subtree is the previous record's (never set on a slab's first record), the operand stays in registers.  A candidate's
// weighted sum: per lane, wave shuffle, the waves of the workgroup through LDS, then ONE 64-bit store per workgroup -- its partial
// of (candidate, tile) -- and pars_regraft_sum adds a candidate's partials with one wave: integers, the same for any grid.  (One
// atomic add per workgroup into the candidate's word was measured first: at 100 000 patterns the 391 adds per word, eight words a
// cache line, bound the kernel -- 42.7 against 10.2 us at 8 candidates; profiles/parsimony_regraft_scan.md.)  The kept candidate's
// J and site scores are stored by the workgroups of its slab, every lane its own patterns.

struct ParsScanParams
{
  ParsParams          q;     // (ops, site, sum, n_ops, score, b1, b2 unused; w: the integer weights, zero behind P)
  const ParsScanRec  *recs;  // [n]
  unsigned long long *sums;  // [n]: written by pars_regraft_sum
  int2               *keep_fitch; // [Pp]
  int                *keep_gen;   // [S][Pp]
  int                *keep_site;  // [Pp]
  int                 n, slab, keep_cand;
  unsigned long long *tile_sums; // [n][tiles]
  int                 tiles;
};

constexpr int kParsScanFitchWaves = kParsTile / 2 / 64, kParsScanGeneralWaves = kParsTile / 64;
constexpr int kParsScanFitchLds = 2 * kParsScanFitchWaves * (int)sizeof(long long);     // capi.py: PARS_REGRAFT_LDS
constexpr int kParsScanGeneralLds = 2 * kParsScanGeneralWaves * (int)sizeof(long long); // ... plus S * S ints

// candidate k's sum over the workgroup; ws[k & 1]: two sets of slots, so that one barrier per candidate is enough (a slot written for
// candidate k is read before the barrier of k + 1 and written again behind it)
template <int NW> __device__ __forceinline__ void pars_scan_sum(long long acc, long long (*ws)[NW], int k, const ParsScanParams &a)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) ws[k & 1][threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += ws[k & 1][w];
    a.tile_sums[(size_t)k * a.tiles + blockIdx.x] = (unsigned long long)s;
  }
}

// a candidate's tile sums added by one wave
__global__ __launch_bounds__(64) void pars_regraft_sum(const unsigned long long *__restrict__ tile_sums, unsigned long long *__restrict__ out, const int tiles)
{
  const unsigned long long *row = tile_sums + (size_t)blockIdx.x * tiles;
  unsigned long long s = 0;
  for (int t = threadIdx.x; t < tiles; t += 64) s += row[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <int S> __global__ __launch_bounds__(kParsTile / 2) void pars_regraft_fitch(const ParsScanParams a)
{
  __shared__ long long ws[2][kParsScanFitchWaves];
  const ParsParams &q = a.q;
  const long long p = ((long long)blockIdx.x * (kParsTile / 2) + threadIdx.x) * 2; // (p + 1 < Pp: Pp is even)
  const bool      in = p < q.P, two = p + 1 < q.P;
  const int       first = (int)blockIdx.y * a.slab, last = first + a.slab < a.n ? first + a.slab : a.n;
  const int4      zero = make_int4(0, 0, 0, 0);
  long long       w0 = 0, w1 = 0;
  int4            c1 = zero, c2 = zero, sub = zero;
  if (in)
  {
    const ParsScanRec r = a.recs[first];
    w0 = q.w[p];
    w1 = two ? q.w[p + 1] : 0ll;
    c1 = fitch_load<S>(q, r.c1, p, two);
    c2 = fitch_load<S>(q, r.c2, p, two);
    sub = fitch_load<S>(q, r.sub, p, two);
  }
  for (int k = first; k < last; ++k)
  {
    int4 n1 = zero, n2 = zero, ns = sub;
    if (k + 1 < last && in)
    { // the next candidate's operands, before this one is reduced
      const ParsScanRec nr = a.recs[k + 1];
      n1 = fitch_load<S>(q, nr.c1, p, two);
      n2 = fitch_load<S>(q, nr.c2, p, two);
      if (!(nr.flags & 1)) ns = fitch_load<S>(q, nr.sub, p, two);
    }
    const int4 j = fitch_join(c1, c2);
    const int  s0 = j.y + sub.y + ((j.x & sub.x) ? 0 : 1), s1 = j.w + sub.w + ((j.z & sub.z) ? 0 : 1); // src/pars.c:432-433
    if (k == a.keep_cand && in)
    {
      *reinterpret_cast<int4 *>(a.keep_fitch + p) = j;
      a.keep_site[p] = s0;
      if (two) a.keep_site[p + 1] = s1;
    }
    pars_scan_sum<kParsScanFitchWaves>((long long)s0 * w0 + (long long)s1 * w1, ws, k, a);
    c1 = n1; c2 = n2; sub = ns;
  }
}

// One row of the min-plus product: min(MAX_PARS, min_j(v[j] + step[i][j])) (src/pars.c:359-375, :411-427); row i of the matrix from
// LDS at a wave-uniform address
template <int S> __device__ __forceinline__ int general_row_min(const int *step, int i, const int (&v)[S])
{
  int x = kMaxPars;
#pragma unroll
  for (int j = 0; j < S; ++j)
  {
    const int t = v[j] + step[i * S + j];
    x = t < x ? t : x;
  }
  return x;
}

// general_load for the scan: the plane's S rows at wave-uniform 64-bit bases plus ONE 32-bit byte offset of the lane (a pattern count
// above 2^30 is refused by the host), so that a load in flight holds no address registers of its own
template <int S> __device__ __forceinline__ void scan_general_load(const ParsParams &q, int b, long long p, unsigned lane_bytes, int (&v)[S])
{
  if (b < q.tips)
  {
    const uint32_t mask = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, b, p);
#pragma unroll
    for (int j = 0; j < S; ++j) v[j] = ((mask >> j) & 1u) ? 0 : kMaxPars;
  }
  else
  {
    const char *plane = reinterpret_cast<const char *>(q.gen + (size_t)(b - q.tips) * S * q.Pp);
#pragma unroll
    for (int j = 0; j < S; ++j) v[j] = *reinterpret_cast<const int *>(plane + (size_t)j * q.Pp * sizeof(int) + lane_bytes);
  }
}

// Registers of a lane: the subtree's S minima, the two children (2 S), J (S).  The children are dead once J is formed: the next
// record's are loaded into their registers in front of the third min-plus product, which hides them.  The loops over i stay loops at
// 20 states, as in general_step (unrolled, the matrix entries are hoisted and spill: tried, 243 spilled registers even with the rows
// fenced off from each other).  general_step's rows go to memory as they are formed; these stay in registers, so J[i] and min_r[i]
// are registers chosen by a wave-uniform index (the index mode, no scratch), and an array indexed that way is a register tuple of
// the next power of two: 32 registers for 20 values.
template <int S> __global__ __launch_bounds__(kParsTile) void pars_regraft_general(const ParsScanParams a)
{
  __shared__ int       step[S * S];
  __shared__ long long ws[2][kParsScanGeneralWaves];
  const ParsParams &q = a.q;
  for (int i = threadIdx.x; i < S * S; i += kParsTile) step[i] = q.step[i];
  __syncthreads();
  const long long p = (long long)blockIdx.x * kParsTile + threadIdx.x;
  const bool      in = p < q.P;
  const long long pl = in ? p : 0; // a lane behind the last pattern reads pattern 0 and weighs it 0: no load below is conditional
  const unsigned  lane_bytes = (unsigned)pl * (unsigned)sizeof(int);
  const int       first = (int)blockIdx.y * a.slab, last = first + a.slab < a.n ? first + a.slab : a.n;
  const long long w = in ? q.w[p] : 0ll;
  constexpr int   kRows = S <= 4 ? S : 1;
  int v1[S], v2[S], min_r[S], J[S];
  {
    const ParsScanRec r = a.recs[first];
    scan_general_load<S>(q, r.sub, pl, lane_bytes, J);
#pragma unroll kRows
    for (int i = 0; i < S; ++i) min_r[i] = general_row_min<S>(step, i, J); // once per subtree, shared by the candidates that follow
    scan_general_load<S>(q, r.c1, pl, lane_bytes, v1);
    scan_general_load<S>(q, r.c2, pl, lane_bytes, v2);
  }
  for (int k = first; k < last; ++k)
  {
#pragma unroll kRows
    for (int i = 0; i < S; ++i) J[i] = general_row_min<S>(step, i, v1) + general_row_min<S>(step, i, v2);
    // the next candidate's children, before this one is scored and reduced (behind the slab's last record: its own once more)
    const ParsScanRec nr = a.recs[k + 1 < last ? k + 1 : k];
    scan_general_load<S>(q, nr.c1, pl, lane_bytes, v1);
    scan_general_load<S>(q, nr.c2, pl, lane_bytes, v2);
    const bool new_sub = k + 1 < last && !(nr.flags & 1);
    if (k == a.keep_cand && in)
    {
#pragma unroll
      for (int i = 0; i < S; ++i) a.keep_gen[(size_t)i * q.Pp + p] = J[i];
    }
    int site = kMaxPars;
#pragma unroll kRows
    for (int i = 0; i < S; ++i)
    {
      const int t = general_row_min<S>(step, i, J) + min_r[i];
      site = t < site ? t : site;
    }
    if (k == a.keep_cand && in) a.keep_site[p] = site;
    pars_scan_sum<kParsScanGeneralWaves>((long long)site * w, ws, k, a);
    if (new_sub)
    { // (wave-uniform: the record is)
      scan_general_load<S>(q, nr.sub, pl, lane_bytes, J);
#pragma unroll kRows
      for (int i = 0; i < S; ++i) min_r[i] = general_row_min<S>(step, i, J);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------

static void pars_free_planes(ParsState *T)
{
  if (T->d_fitch) (void)hipFree(T->d_fitch);
  if (T->d_gen) (void)hipFree(T->d_gen);
  if (T->d_step) (void)hipFree(T->d_step);
  T->d_fitch = nullptr;
  T->d_gen = T->d_step = nullptr;
}

void pars_release(Instance *I)
{
  ParsState *T = I->pars;
  if (!T) return;
  pars_free_planes(T);
  T->scan.work.release();
  void *dev[] = {T->d_site, T->d_w, T->d_sum, T->d_ops[0], T->d_ops[1]};
  for (void *x : dev)
    if (x) (void)hipFree(x);
  void *host[] = {T->h_sum, T->h_ops[0], T->h_ops[1]};
  for (void *x : host)
    if (x) (void)hipHostFree(x);
  for (hipEvent_t e : T->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &pr : T->prof_pairs)
  {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  delete T;
  I->pars = nullptr;
}

// the refusals that belong to the kind of instance, then "not enabled"
static int pars_gate(const Instance *I, const char *who, bool need_state)
{
  if (const int rc = refuse_kind(I, who, kRefuseRank | kRefuseClassAxis | kRefuseStates)) return rc;
  if (need_state && !I->pars) return fail(PHYHIP_ERROR_UNINITIALIZED_INSTANCE, "%s before phyhip_set_parsimony", who);
  return 0;
}

static int pars_collect_profile(Instance *I)
{
  ParsState *T = I->pars;
  if (T->prof_pairs.empty()) return 0;
  HIPCHK(hipStreamSynchronize(I->stream));
  for (auto &pr : T->prof_pairs)
  {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) T->prof_ms += (double)ms;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  T->prof_pairs.clear();
  return 0;
}

// one launch: what is queued, then -- score -- the edge (b1, b2); with_sum: the weighted sum into d_sum and on to h_sum
static int pars_launch(Instance *I, bool score, int b1, int b2, bool with_sum)
{
  ParsState *T = I->pars;
  const int  n = (int)T->pending.size();
  if (n == 0 && !score) return 0;
  int rc;
  if (I->S > 8 && (rc = upload_masks(I))) return rc;
  const int s = T->slot;
  T->slot ^= 1;
  if (T->ev_pending[s])
  { // the launch that last read this slot's host copy
    HIPCHK(hipEventSynchronize(T->ev[s]));
    T->ev_pending[s] = false;
  }
  if (n > 0)
  {
    memcpy(T->h_ops[s], T->pending.data(), (size_t)n * sizeof(int4));
    HIPCHK(hipMemcpyAsync(T->d_ops[s], T->h_ops[s], (size_t)n * sizeof(int4), hipMemcpyHostToDevice, I->stream));
  }
  if (score && with_sum) HIPCHK(hipMemsetAsync(T->d_sum, 0, sizeof(unsigned long long), I->stream));
  ParsParams q;
  memset(&q, 0, sizeof q);
  q.tip_codes = I->d_tipcodes; q.code_masks = I->d_masks; q.fitch = T->d_fitch; q.gen = T->d_gen; q.step = T->d_step;
  q.ops = T->d_ops[s]; q.site = T->d_site; q.w = (score && with_sum) ? T->d_w : nullptr; q.sum = T->d_sum;
  q.P = I->P; q.Pp = T->Pp; q.Ppad = I->Ppad; q.n_ops = n; q.tips = I->tips; q.score = score ? 1 : 0; q.b1 = b1; q.b2 = b2;
  SideTimer tm(I); // (its pair goes to prof_pairs: collected when the profile is read)
  if ((rc = tm.tic())) return rc;
  const dim3 grid((unsigned)((I->P + kParsTile - 1) / kParsTile));
  if (!T->general)
  {
    if (I->S == 4) hipLaunchKernelGGL(pars_fitch_kernel<4>, grid, dim3(kParsTile / 2), 0, I->stream, q);
    else hipLaunchKernelGGL(pars_fitch_kernel<20>, grid, dim3(kParsTile / 2), 0, I->stream, q);
  }
  else
  {
    if (I->S == 4) hipLaunchKernelGGL(pars_general_kernel<4>, grid, dim3(kParsTile), 0, I->stream, q);
    else hipLaunchKernelGGL(pars_general_kernel<20>, grid, dim3(kParsTile), 0, I->stream, q);
  }
  HIPCHK(hipGetLastError());
  if (I->prof)
  {
    if ((rc = tm.mark())) return rc;
    T->prof_pairs.push_back(tm.detach());
    ++T->prof_n;
    T->prof_updates += (double)I->P * (double)(n + (score ? 1 : 0));
  }
  HIPCHK(hipEventRecord(T->ev[s], I->stream));
  T->ev_pending[s] = true;
  if (score && with_sum) HIPCHK(hipMemcpyAsync(T->h_sum, T->d_sum, sizeof(unsigned long long), hipMemcpyDeviceToHost, I->stream));
  T->pending.clear();
  T->last_dest = -1;
  if (score) T->scored = true;
  return 0;
}

// (phyhip_synchronize: what is queued here runs too)
int pars_flush_queue(Instance *I) { return I->pars ? pars_launch(I, false, 0, 0, false) : 0; }

static int pars_set(Instance *I, int general, const int *step)
{
  static const char *const who = "phyhip_set_parsimony";
  int rc;
  if ((rc = pars_gate(I, who, false))) return rc;
  if (general && !step) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: the step-matrix mode needs a step matrix", who);
  ParsState *T = I->pars;
  if (!T)
  {
    T = I->pars = new ParsState;
    T->Pp = (I->P + 1) & ~1ll;
    T->ninner = I->nbuf - I->tips;
    const size_t Pp = (size_t)T->Pp;
    if ((rc = side_alloc((void **)&T->d_site, Pp * sizeof(int), who))) return rc;
    if ((rc = side_alloc((void **)&T->d_w, Pp * sizeof(long long), who))) return rc;
    if ((rc = side_alloc((void **)&T->d_sum, sizeof(unsigned long long), who))) return rc;
    HIPCHK(hipMemset(T->d_site, 0, Pp * sizeof(int)));
    HIPCHK(hipMemset(T->d_w, 0, Pp * sizeof(long long)));
    HIPCHK(hipHostMalloc((void **)&T->h_sum, sizeof(unsigned long long), hipHostMallocDefault));
    for (int s = 0; s < 2; ++s)
    {
      if ((rc = side_alloc((void **)&T->d_ops[s], (size_t)kParsStaging * sizeof(int4), who))) return rc;
      HIPCHK(hipHostMalloc((void **)&T->h_ops[s], (size_t)kParsStaging * sizeof(int4), hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&T->ev[s], hipEventDisableTiming));
    }
    T->general = -1; // (no planes yet)
  }
  else
  { // what was queued belongs to the mode it was queued in
    if (T->general >= 0 && (rc = pars_launch(I, false, 0, 0, false))) return rc;
    HIPCHK(hipStreamSynchronize(I->stream));
  }
  const int    mode = general ? 1 : 0;
  const size_t Pp = (size_t)T->Pp, S = (size_t)I->S, nin = (size_t)(T->ninner > 0 ? T->ninner : 1);
  if (T->general != mode)
  {
    pars_free_planes(T);
    T->general = -1;
    T->scored = false;
    T->scan.keep_valid = false; // (the kept plane of a regraft scan has the other mode's shape)
    if (mode == 0)
    {
      if ((rc = side_alloc((void **)&T->d_fitch, nin * Pp * sizeof(int2), who))) return rc;
      HIPCHK(hipMemset(T->d_fitch, 0, nin * Pp * sizeof(int2)));
    }
    else
    {
      if ((rc = side_alloc((void **)&T->d_gen, nin * S * Pp * sizeof(int), who))) return rc;
      if ((rc = side_alloc((void **)&T->d_step, S * S * sizeof(int), who))) return rc;
      HIPCHK(hipMemset(T->d_gen, 0, nin * S * Pp * sizeof(int)));
    }
    T->general = mode;
  }
  if (mode == 1) HIPCHK(hipMemcpy(T->d_step, step, S * S * sizeof(int), hipMemcpyHostToDevice));
  T->w_epoch = ~0ull; // the integer weights are made again
  return PHYHIP_SUCCESS;
}

static int pars_queue(Instance *I, const phyhip_parsimony_operation *ops, int count)
{
  static const char *const who = "phyhip_update_partial_parsimony";
  int rc;
  if ((rc = pars_gate(I, who, true))) return rc;
  if (count < 0 || (count > 0 && !ops)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: %d operations", who, count);
  for (int k = 0; k < count; ++k)
  {
    if ((rc = check_partial_index(I, ops[k].destination, false))) return rc;
    if ((rc = check_partial_index(I, ops[k].child1, true))) return rc;
    if ((rc = check_partial_index(I, ops[k].child2, true))) return rc;
    if (ops[k].destination == ops[k].child1 || ops[k].destination == ops[k].child2)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: operation %d writes buffer %d, which it reads", who, k, ops[k].destination);
  }
  ParsState *T = I->pars;
  for (int k = 0; k < count; ++k)
  {
    if ((int)T->pending.size() == kParsStaging && (rc = pars_launch(I, false, 0, 0, false))) return rc;
    const int flags = (ops[k].child1 == T->last_dest ? 1 : 0) | (ops[k].child2 == T->last_dest ? 2 : 0);
    T->pending.push_back(make_int4(ops[k].destination, ops[k].child1, ops[k].child2, flags));
    T->last_dest = ops[k].destination;
  }
  return PHYHIP_SUCCESS;
}

// the instance's pattern weights as integers, made again after every phyhip_set_pattern_weights (Instance::wght_epoch); which are
// written synchronously, behind a flush: nothing on the stream changes them
static int pars_weights(Instance *I)
{
  ParsState *T = I->pars;
  if (T->w_epoch == I->wght_epoch) return 0;
  std::vector<double>    w((size_t)I->P);
  std::vector<long long> wi((size_t)T->Pp, 0ll);
  HIPCHK(hipStreamSynchronize(I->stream)); // (a scoring kernel still reading the old integers)
  HIPCHK(hipMemcpy(w.data(), I->d_wght, (size_t)I->P * sizeof(double), hipMemcpyDeviceToHost));
  T->w_integer = true;
  for (long long p = 0; p < I->P; ++p)
  {
    const double x = w[(size_t)p];
    if (!(std::fabs(x) < 9007199254740992.0) || x != std::floor(x)) { T->w_integer = false; break; }
    wi[(size_t)p] = (long long)x;
  }
  if (T->w_integer) HIPCHK(hipMemcpy(T->d_w, wi.data(), (size_t)T->Pp * sizeof(long long), hipMemcpyHostToDevice));
  T->w_epoch = I->wght_epoch;
  return 0;
}

// every check of a scoring call, before any device work of any shard
static int pars_score_check(Instance *I, int b1, int b2, bool with_sum)
{
  static const char *const who = "phyhip_calculate_edge_parsimony";
  int rc;
  if ((rc = pars_gate(I, who, true))) return rc;
  if ((rc = check_partial_index(I, b1, true)) || (rc = check_partial_index(I, b2, true))) return rc;
  if (with_sum)
  {
    if ((rc = pars_weights(I))) return rc;
    if (!I->pars->w_integer)
      return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: a pattern weight is not an integer (pass outParsimony = NULL and add site_pars * wght on the host)", who);
  }
  return 0;
}

static int pars_wait_sum(Instance *I, long long *sum)
{
  HIPCHK(hipStreamSynchronize(I->stream));
  if (sum) *sum += (long long)*I->pars->h_sum;
  return 0;
}

static int pars_get_site(Instance *I, int *out)
{
  int rc;
  if ((rc = pars_gate(I, "phyhip_get_site_parsimony", true))) return rc;
  if (!I->pars->scored) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_get_site_parsimony: no edge was scored yet");
  if ((rc = pars_launch(I, false, 0, 0, false))) return rc;
  HIPCHK(hipStreamSynchronize(I->stream));
  HIPCHK(hipMemcpy(out, I->pars->d_site, (size_t)I->P * sizeof(int), hipMemcpyDeviceToHost));
  return PHYHIP_SUCCESS;
}

static int pars_get_partial(Instance *I, int buf, int *ui, int *pars, int *ppars)
{
  static const char *const who = "phyhip_get_partial_parsimony";
  int rc;
  if ((rc = pars_gate(I, who, true))) return rc;
  if ((rc = check_partial_index(I, buf, false))) return rc;
  ParsState *T = I->pars;
  if (T->general ? (ui || pars) : (ppars != nullptr))
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: %s", who, T->general ? "the step-matrix mode holds no ui / pars" : "the Fitch mode holds no p_pars");
  if ((rc = pars_launch(I, false, 0, 0, false))) return rc;
  HIPCHK(hipStreamSynchronize(I->stream));
  const size_t P = (size_t)I->P, Pp = (size_t)T->Pp, S = (size_t)I->S, k = (size_t)(buf - I->tips);
  if (!T->general)
  {
    std::vector<int2> h(Pp);
    HIPCHK(hipMemcpy(h.data(), T->d_fitch + k * Pp, Pp * sizeof(int2), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < P; ++p)
    {
      if (ui) ui[p] = h[p].x;
      if (pars) pars[p] = h[p].y;
    }
  }
  else if (ppars)
  {
    std::vector<int> h(S * Pp);
    HIPCHK(hipMemcpy(h.data(), T->d_gen + k * S * Pp, S * Pp * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < P; ++p)
      for (size_t s = 0; s < S; ++s) ppars[p * S + s] = h[s * Pp + p];
  }
  return PHYHIP_SUCCESS;
}

// ---- regraft scan: host side -------------------------------------------------------------------------------------------------------

static const char *const kParsScan = "phyhip_calculate_regraft_parsimony";

// every check of a scan, before any device work of any shard
static int pars_scan_check(Instance *I, const phyhip_parsimony_candidate *cand, int count)
{
  int rc;
  if ((rc = pars_gate(I, kParsScan, true))) return rc;
  if (I->P > (1ll << 30)) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for more than 2^30 patterns (%lld)", kParsScan, I->P);
  for (int k = 0; k < count; ++k)
    if ((rc = check_partial_index(I, cand[k].child1, true)) || (rc = check_partial_index(I, cand[k].child2, true)) ||
        (rc = check_partial_index(I, cand[k].subtree, true)))
      return fail(rc, "%s: candidate %d: %s", kParsScan, k, std::string(g_err).c_str());
  if (count == 0) return 0;
  if ((rc = pars_weights(I))) return rc;
  if (!I->pars->w_integer)
    return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: a pattern weight is not an integer (score the candidates edge by edge and add site_pars * wght on the host)", kParsScan);
  return 0;
}

// what is queued, then the candidates in chunks: one copy up, the scan kernel and the sum kernel, one wait and one copy down each;
// sums[k]: this shard's
static int pars_scan_run(Instance *I, const phyhip_parsimony_candidate *cand, int count, int keep, long long *sums)
{
  ParsState *T = I->pars;
  auto      &U = T->scan;
  int        rc;
  U.keep_valid = false;
  if (count == 0) return 0;
  if ((rc = pars_launch(I, false, 0, 0, false))) return rc; // (the path updates of the caller, in stream order)
  if (I->S > 8 && (rc = upload_masks(I))) return rc;
  U.lay = ParsScanLayout((size_t)I->P, (size_t)I->S, T->general != 0, std::min((size_t)count, kScanGridCap));
  const ParsScanLayout &L = U.lay;
  if ((rc = U.work.reserve(L.total, kParsScan))) return rc;
  ParsScanParams a;
  memset(&a, 0, sizeof a);
  a.q.tip_codes = I->d_tipcodes; a.q.code_masks = I->d_masks; a.q.fitch = T->d_fitch; a.q.gen = T->d_gen; a.q.step = T->d_step;
  a.q.w = T->d_w; a.q.P = I->P; a.q.Pp = T->Pp; a.q.Ppad = I->Ppad; a.q.tips = I->tips;
  ParsScanRec *const d_recs = U.work.at<ParsScanRec>(L.recs);
  a.recs = d_recs; a.sums = U.work.at<unsigned long long>(L.sums);
  a.keep_fitch = U.work.at<int2>(L.keep); a.keep_gen = U.work.at<int>(L.keep); a.keep_site = U.work.at<int>(L.site);
  const size_t tiles = (size_t)((I->P + kParsTile - 1) / kParsTile);
  a.tile_sums = U.work.at<unsigned long long>(L.tile_sums); a.tiles = (int)tiles;
  SideTimer    tm(I);
  rc = for_each_chunk(count, L.chunk, keep, [&](size_t first, size_t n, int keep_cand) {
    const ParsScanSlabs slabs(n, tiles, (size_t)(I->cus > 0 ? I->cus : 256));
    U.recs.resize(n);
    for (size_t k = 0; k < n; ++k)
    {
      const phyhip_parsimony_candidate &c = cand[first + k];
      U.recs[k] = ParsScanRec{c.child1, c.child2, c.subtree, (k % slabs.size != 0 && c.subtree == cand[first + k - 1].subtree) ? 1 : 0};
    }
    HIPCHK(hipMemcpyAsync(d_recs, U.recs.data(), n * sizeof(ParsScanRec), hipMemcpyHostToDevice, I->stream));
    a.n = (int)n; a.slab = (int)slabs.size; a.keep_cand = keep_cand;
    const dim3 grid((unsigned)tiles, (unsigned)slabs.count);
    const int  rt = side_timed(tm, I, U.prof_ms, [&] {
      if (!T->general)
      {
        if (I->S == 4) hipLaunchKernelGGL(pars_regraft_fitch<4>, grid, dim3(kParsTile / 2), 0, I->stream, a);
        else hipLaunchKernelGGL(pars_regraft_fitch<20>, grid, dim3(kParsTile / 2), 0, I->stream, a);
      }
      else
      {
        if (I->S == 4) hipLaunchKernelGGL(pars_regraft_general<4>, grid, dim3(kParsTile), 0, I->stream, a);
        else hipLaunchKernelGGL(pars_regraft_general<20>, grid, dim3(kParsTile), 0, I->stream, a);
      }
      hipLaunchKernelGGL(pars_regraft_sum, dim3((unsigned)n), dim3(64), 0, I->stream, a.tile_sums, a.sums, a.tiles);
      return 0;
    });
    if (rt) return rt;
    U.down.resize(n);
    HIPCHK(hipMemcpy(U.down.data(), a.sums, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) sums[first + k] = (long long)U.down[k];
    return 0;
  });
  if (rc) return rc;
  U.keep_valid = keep >= 0;
  if (I->prof) ++U.prof_n, U.prof_cand += count;
  return 0;
}

static int pars_scan_kept(Instance *I, const char *who)
{
  if (const int rc = pars_gate(I, who, true)) return rc;
  const auto &U = I->pars->scan;
  if (!U.keep_valid || !U.work.ptr) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: no %s call before it that kept a candidate", who, kParsScan);
  return 0;
}

static int pars_scan_get_site(Instance *I, int *out)
{
  if (const int rc = pars_scan_kept(I, "phyhip_get_regraft_site_parsimony")) return rc;
  const auto &U = I->pars->scan;
  HIPCHK(hipMemcpy(out, U.work.at<int>(U.lay.site), (size_t)I->P * sizeof(int), hipMemcpyDeviceToHost));
  return PHYHIP_SUCCESS;
}

static int pars_scan_get_partial(Instance *I, int *ui, int *pars, int *ppars)
{
  static const char *const who = "phyhip_get_regraft_partial_parsimony";
  if (const int rc = pars_scan_kept(I, who)) return rc;
  ParsState *T = I->pars;
  if (T->general ? (ui || pars) : (ppars != nullptr))
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: %s", who, T->general ? "the step-matrix mode holds no ui / pars" : "the Fitch mode holds no p_pars");
  const auto  &U = T->scan;
  const size_t P = (size_t)I->P, Pp = U.lay.Pp, S = (size_t)I->S;
  if (!T->general)
  {
    std::vector<int2> h(Pp);
    HIPCHK(hipMemcpy(h.data(), U.work.at<int2>(U.lay.keep), Pp * sizeof(int2), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < P; ++p)
    {
      if (ui) ui[p] = h[p].x;
      if (pars) pars[p] = h[p].y;
    }
  }
  else if (ppars)
  {
    std::vector<int> h(S * Pp);
    HIPCHK(hipMemcpy(h.data(), U.work.at<int>(U.lay.keep), S * Pp * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < P; ++p)
      for (size_t s = 0; s < S; ++s) ppars[p * S + s] = h[s * Pp + p];
  }
  return PHYHIP_SUCCESS;
}

static int pars_profile_gate(Instance *I, double *ms, int *n, double *up)
{
  int rc;
  if ((rc = pars_gate(I, "phyhip_profile_read_parsimony", true)) || (rc = pars_collect_profile(I))) return rc;
  ParsState *T = I->pars;
  if (T->prof_ms > *ms) *ms = T->prof_ms; // (shards: the slowest one's kernels)
  if (T->prof_n > *n) *n = T->prof_n;
  *up += T->prof_updates;
  T->prof_ms = T->prof_updates = 0.0;
  T->prof_n = 0;
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

// Every entry point here walks the plain instance or every shard as a QUERY (nothing here is a step of the sequence the resident
// evaluators watch, and nothing it puts on the stream touches what they read), and looks a group up without draining the queue-only
// likelihood calls it has recorded: they stay recorded.

int phyhip_set_parsimony(int instance, int general, const int *stepMatrix)
{
  return side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long, long long) { return pars_set(I, general, stepMatrix); });
}

int phyhip_update_partial_parsimony(int instance, const phyhip_parsimony_operation *ops, int count)
{
  return side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long, long long) { return pars_queue(I, ops, count); });
}

int phyhip_calculate_edge_parsimony(int instance, int buffer1, int buffer2, long long *outParsimony)
{
  const bool with_sum = outParsimony != nullptr;
  long long  sum = 0;
  // three passes: every check of every shard, then every launch, then every wait
  int rc = side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long, long long) { return pars_score_check(I, buffer1, buffer2, with_sum); });
  if (rc < 0) return rc;
  rc = side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long, long long) { return pars_launch(I, true, buffer1, buffer2, with_sum); });
  if (rc < 0) return rc;
  rc = side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long, long long) { return pars_wait_sum(I, with_sum ? &sum : nullptr); });
  if (rc < 0) return rc;
  if (outParsimony) *outParsimony = sum;
  return PHYHIP_SUCCESS;
}

int phyhip_get_site_parsimony(int instance, int *outSitePars)
{
  if (!outSitePars) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_get_site_parsimony: a NULL array");
  return side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long lo, long long) { return pars_get_site(I, outSitePars + lo); });
}

int phyhip_get_partial_parsimony(int instance, int bufferIndex, int *outUi, int *outPars, int *outPPars)
{
  return side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long lo, long long) {
    return pars_get_partial(I, bufferIndex, outUi ? outUi + lo : nullptr, outPars ? outPars + lo : nullptr, outPPars ? outPPars + lo * I->S : nullptr);
  });
}

int phyhip_profile_read_parsimony(int instance, double *outKernelMs, int *outLaunches, double *outPatternUpdates)
{
  double ms = 0.0, up = 0.0;
  int    n = 0;
  const int rc = side_each<kSideNoDrain, kSideQuery>(instance, [&](Instance *I, long long, long long) { return pars_profile_gate(I, &ms, &n, &up); });
  if (rc < 0) return rc;
  if (outKernelMs) *outKernelMs = ms;
  if (outLaunches) *outLaunches = n;
  if (outPatternUpdates) *outPatternUpdates = up;
  return PHYHIP_SUCCESS;
}

// A scan, unlike the six calls above, is a call that puts work on the stream: it enters as the other candidate-list calls do (the
// group drained, the large-grid resident workgroups leave), every shard checked before any shard runs.

int phyhip_calculate_regraft_parsimony(int instance, const phyhip_parsimony_candidate *candidates, int count, int keepCandidate, long long *outParsimony)
{
  if (count < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate count %d", kParsScan, count);
  if (count > 0 && (!candidates || !outParsimony)) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: a NULL array for %d candidates", kParsScan, count);
  if (keepCandidate < -1 || keepCandidate >= count) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: keepCandidate %d of %d candidates", kParsScan, keepCandidate, count);
  SideShards s;
  int rc = side_collect(instance, kParsScan, kRefuseRank | kRefuseClassAxis | kRefuseStates, s);
  if (rc < 0) return rc;
  for (Instance *I : s.sh)
    if ((rc = pars_scan_check(I, candidates, count))) return rc;
  std::vector<long long> part((size_t)count), sum((size_t)count, 0ll);
  for (Instance *I : s.sh)
  { // every shard scans its pattern range; the integer sums are added
    if ((rc = pars_scan_run(I, candidates, count, keepCandidate, part.data()))) return rc;
    for (size_t k = 0; k < sum.size(); ++k) sum[k] += part[k];
  }
  std::copy(sum.begin(), sum.end(), outParsimony);
  return PHYHIP_SUCCESS;
}

int phyhip_get_regraft_site_parsimony(int instance, int *outSitePars)
{
  if (!outSitePars) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_get_regraft_site_parsimony: a NULL array");
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long) { return pars_scan_get_site(I, outSitePars + lo); });
}

int phyhip_get_regraft_partial_parsimony(int instance, int *outUi, int *outPars, int *outPPars)
{
  return side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long) {
    return pars_scan_get_partial(I, outUi ? outUi + lo : nullptr, outPars ? outPars + lo : nullptr, outPPars ? outPPars + lo * I->S : nullptr);
  });
}

// read and reset: the time is added over the shards; calls and candidates are the same on every shard, the first one's are taken
int phyhip_profile_read_regraft_parsimony(int instance, double *outKernelMs, int *outCalls, long long *outCandidates)
{
  double    ms = 0.0;
  int       n = 0;
  long long nc = 0;
  bool      first = true;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    if (const int r = pars_gate(I, "phyhip_profile_read_regraft_parsimony", true)) return r;
    auto &U = I->pars->scan;
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

} // extern "C"
