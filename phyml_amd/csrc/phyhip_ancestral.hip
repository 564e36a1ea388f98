// phyhip_ancestral.hip -- the marginal posterior of every state at internal nodes: phyhip_calculate_node_state_posteriors
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
//
// Ancestral_Sequences_One_Node (src/ancestral.c:609-901) reads, for an internal node d and a pattern p, the three directional
// partial vectors that meet at d -- the one of edge b_k on neighbour v_k's side, k = 0..2 -- and forms per state i
//   x_k(c,i) = sum_j side_k[p][c][j] * Pij_k[c][i][j]         (a tip: its 0/1 vector, the same in every category)
//   q[i]     = sum_c x_0 x_1 x_2 pi[i] gamma_r_proba[c]        ss = the sum of the non-tip sides' scale exponents at p
//   +I:        q[i] = q[i] (1 - pinvar) + Invariant_Lk(ss, p) pinvar pi[i], or Invariant_Lk(0, p) pinvar pi[i] where that overflowed
//   post[i]  = exp(log(q[i]) - LOG2 ss - c_lnL_sorted[p])
// A binding used to download all 3(n-2) partial and scale vectors of the tree for this loop; here one launch serves a list of
// nodes, grid (pattern tiles of 256, node), one lane per pattern, and only the answer -- [node][pattern][state] -- crosses the link.
//
// NO bit parity with the reference's binary is claimed for this call: its products run in plain C order under -O3 contraction,
// which nothing here pins, so the inner products below are fused chains and the order of additions is this kernel's own.  The
// tests hold it to a numpy restatement of the formula at 1e-10 relative (tests/ancestral_ref.py), the restatement to the
// reference's printed probabilities.  log and exp are the reference's libm's (phyhip_log.hpp, phyhip_exp.hpp).
// It writes a work space of its own: what the evaluation kernels left (site outputs, warning flag, results) stays as it was.
#include "phyhip_side.hpp"
#include "phyhip_layout.hpp"
#include "phyhip_log.hpp"

namespace phyhip_host
{

struct AncParams
{
  const uint8_t  *tip_codes;
  const uint32_t *code_masks;
  const double   *wght, *pi, *cat_w;
  const short    *invar;
  const double   *pmats;    // the instance's matrix table
  const double   *partials;
  const int      *scales;
  const int      *nodes;    // [node][6]: the three side indices (partials buffer or tip), then the three matrix indices
  const double   *site_lnl; // [P]
  double         *out;      // [node][P][S]
  int            *warn;     // [1]
  long long       P, Ppad;
  int             C, tips, layout, apply_scaling, invar_model;
  double          pinvar;
};

// One lane per pattern, one node per blockIdx.y (what kind of neighbour sits behind each edge is the same for the whole
// workgroup).  4 states: the matrices are read at wave-uniform addresses.  20 states: the three matrices of a category (1200
// doubles) are staged in LDS by the workgroup, category after category -- every lane of the workgroup takes part in the barriers,
// also those without a pattern or without weight.
template <int S>
__global__ __launch_bounds__(256) void node_posterior_kernel(const AncParams q)
{
  __shared__ double Ms[S == 20 ? 3 * 400 : 2];
  const long long   p = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool        in = p < q.P;
  const bool        act = in && q.wght[p] > kSmall;
  const int *__restrict__ nd = q.nodes + (size_t)blockIdx.y * 6;
  double acc[S];
#pragma unroll
  for (int i = 0; i < S; ++i) acc[i] = 0.0;

  for (int c = 0; c < q.C; ++c)
  {
    if (S == 20)
    {
      __syncthreads();
      for (int k = 0; k < 3; ++k)
      {
        const double *__restrict__ Mk = q.pmats + ((size_t)nd[3 + k] * q.C + c) * S * S;
        for (int i = threadIdx.x; i < S * S; i += 256) Ms[k * S * S + i] = Mk[i];
      }
      __syncthreads();
    }
    if (!act) continue;
    double prod[S];
#pragma unroll
    for (int i = 0; i < S; ++i) prod[i] = 1.0;
    // (one side after the other, not unrolled: the side vector, the running product and the accumulators are what a lane holds)
#pragma unroll 1
    for (int k = 0; k < 3; ++k)
    {
      const int side = nd[k];
      double    x[S];
      if (side < q.tips)
      {
        const uint32_t m = tip_state_mask<S>(q.tip_codes, q.code_masks, q.Ppad, side, p);
#pragma unroll
        for (int j = 0; j < S; ++j) x[j] = ((m >> j) & 1u) ? 1.0 : 0.0;
      }
      else
      {
#pragma unroll
        for (int j = 0; j < S; ++j) x[j] = q.partials[partial_off<S>(q.layout, q.P, q.Ppad, q.C, side - q.tips, p, c, j)];
      }
      const double *__restrict__ Mk = q.pmats + ((size_t)nd[3 + k] * q.C + c) * S * S; // rows: the state at the node
      const double *Ml = Ms + k * S * S;
#pragma unroll
      for (int i = 0; i < S; ++i)
      {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) a = __builtin_fma(x[j], S == 20 ? Ml[i * S + j] : Mk[i * S + j], a);
        prod[i] = prod[i] * a;
      }
    }
    const double w = q.cat_w[c];
#pragma unroll
    for (int i = 0; i < S; ++i) acc[i] = acc[i] + prod[i] * q.pi[i] * w; // src/ancestral.c:814-819
  }

  if (!in) return;
  double *__restrict__ o = q.out + ((size_t)blockIdx.y * q.P + (size_t)p) * S;
  if (!act)
  { // the reference reads stale vectors at such a pattern; here its row is zero
#pragma unroll
    for (int i = 0; i < S; ++i) o[i] = 0.0;
    return;
  }
  int ss = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (nd[k] >= q.tips) ss += q.scales[(size_t)(nd[k] - q.tips) * q.Ppad + p];
  if (q.invar_model)
  { // src/ancestral.c:843-865 with Invariant_Lk, src/lk.c:1226-1273
    const int iv = q.invar[p];
    double    inv = 0.0;
    bool      issue = false;
    if (iv >= 0) invariant_lk(inv, issue, q.pi[iv], ss, q.apply_scaling);
    if (issue)
    {
      *q.warn = 1;
      const double t = q.pi[iv] * q.pinvar; // Invariant_Lk(0, p)
#pragma unroll
      for (int i = 0; i < S; ++i) acc[i] = t * q.pi[i];
    }
    else
    {
      const double t = inv * q.pinvar;
#pragma unroll
      for (int i = 0; i < S; ++i) acc[i] = acc[i] * (1.0 - q.pinvar) + t * q.pi[i];
    }
  }
  const double shift = kLog2 * (double)ss, lnl = q.site_lnl[p];
#pragma unroll
  for (int i = 0; i < S; ++i) // src/ancestral.c:868-870
    o[i] = phyhip_exp_ref((phyhip_log_ref(acc[i], phyhip_log_data) - shift) - lnl, phyhip_exp_tab);
}

// One plain instance: its patterns of every node into out, the row of node k at out + k * out_pitch (elements)
static int anc_run(Instance *I, int n, const int *sides, const int *mats, const double *lnl, double *out, size_t out_pitch, int *warn_out)
{
  static const char *const who = "phyhip_calculate_node_state_posteriors";
  int rc;
  if ((rc = refuse_kind(I, who, kRefuseClassAxis | kRefuseGenericLoop))) return rc;
  if (I->C < 1 || I->C > kMaxCategories) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d categories", who, I->C);
  if ((rc = refuse_kind(I, who, kRefuseStates))) return rc;
  for (int k = 0; k < 3 * n; ++k)
  {
    if ((rc = check_partial_index(I, sides[k], true))) return rc;
    if (mats[k] < 0 || mats[k] >= I->nmat) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "matrix index %d", mats[k]);
  }
  for (int k = 0; k < 3 * n; ++k) devirtualise(I, sides[k]);
  if ((rc = flush_sync(I))) return rc;
  if ((rc = upload_masks(I))) return rc;
  // work space: the result, the caller's site log-likelihoods, the node table, the flag
  const size_t P = (size_t)I->P, S = (size_t)I->S, n_out = (size_t)n * P * S;
  auto &U = side_of(I).anc;
  if ((rc = U.work.reserve((n_out + P) * sizeof(double) + ((size_t)n * 6 + 1) * sizeof(int), who))) return rc;
  AncParams q;
  memset(&q, 0, sizeof q);
  q.out = (double *)U.work.ptr;
  double *d_lnl = q.out + n_out;
  int    *d_nodes = (int *)(d_lnl + P);
  q.warn = d_nodes + (size_t)n * 6;
  std::vector<int> tab((size_t)n * 6);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < 3; ++j)
    {
      tab[(size_t)k * 6 + j]     = sides[3 * k + j];
      tab[(size_t)k * 6 + 3 + j] = mats[3 * k + j];
    }
  HIPCHK(hipMemcpyAsync(d_nodes, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, I->stream));
  if (lnl) HIPCHK(hipMemcpyAsync(d_lnl, lnl, P * sizeof(double), hipMemcpyHostToDevice, I->stream));
  HIPCHK(hipMemsetAsync(q.warn, 0, sizeof(int), I->stream));
  q.tip_codes = I->d_tipcodes; q.code_masks = I->d_masks; q.wght = I->d_wght; q.pi = I->d_pi; q.cat_w = I->d_catw; q.invar = I->d_invar;
  q.pmats = I->d_pmats; q.partials = I->d_partials; q.scales = I->d_scales;
  q.site_lnl = lnl ? d_lnl : I->d_site_lnl; // (NULL: what the last edge evaluation left, read where it lies)
  q.P = I->P; q.Ppad = I->Ppad; q.C = I->C; q.tips = I->tips; q.layout = layout_of(I);
  q.apply_scaling = I->apply_scaling; q.invar_model = I->invar_model; q.pinvar = I->pinvar;
  SideTimer tm(I);
  if ((rc = tm.tic())) return rc;
  const unsigned tiles = (unsigned)((I->P + 255) / 256);
  for (int first = 0; first < n; first += 65535)
  { // (a grid's second dimension holds 65535 nodes)
    AncParams qc = q;
    qc.nodes = d_nodes + (size_t)first * 6;
    qc.out   = q.out + (size_t)first * P * S;
    const dim3 grid(tiles, (unsigned)(n - first < 65535 ? n - first : 65535)), block(256);
    if (I->S == 4) hipLaunchKernelGGL(node_posterior_kernel<4>, grid, block, 0, I->stream, qc);
    else hipLaunchKernelGGL(node_posterior_kernel<20>, grid, block, 0, I->stream, qc);
    HIPCHK(hipGetLastError());
  }
  if ((rc = tm.mark())) return rc;
  HIPCHK(hipStreamSynchronize(I->stream));
  if ((rc = tm.toc(U.prof_ms))) return rc;
  if (I->prof) ++U.prof_n;
  if (out_pitch == P * S) HIPCHK(hipMemcpy(out, q.out, n_out * sizeof(double), hipMemcpyDeviceToHost));
  else
    HIPCHK(hipMemcpy2D(out, out_pitch * sizeof(double), q.out, P * S * sizeof(double), P * S * sizeof(double), (size_t)n, hipMemcpyDeviceToHost));
  int w = 0;
  HIPCHK(hipMemcpy(&w, q.warn, sizeof(int), hipMemcpyDeviceToHost));
  if (w) *warn_out = 1;
  return PHYHIP_SUCCESS;
}

} // namespace phyhip_host

using namespace phyhip_host;

extern "C" {

int phyhip_calculate_node_state_posteriors(int instance, int nodeCount, const int *sideBufferIndices, const int *probabilityIndices,
                                           const double *inSiteLogLikelihoods, double *outPosteriors, int *outNumericalWarning)
{
  if (nodeCount < 0) return fail(PHYHIP_ERROR_OUT_OF_RANGE, "node count %d", nodeCount);
  if (nodeCount > 0 && (!sideBufferIndices || !probabilityIndices || !outPosteriors))
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "phyhip_calculate_node_state_posteriors: a NULL array for %d nodes", nodeCount);
  int warn = 0;
  if (nodeCount == 0)
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
  }
  else
  {
    const Group *const G = get_group_nodrain(instance); // (for the pitch of the whole only)
    const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long) {
      return anc_run(I, nodeCount, sideBufferIndices, probabilityIndices, inSiteLogLikelihoods ? inSiteLogLikelihoods + lo : nullptr,
                     outPosteriors + (size_t)lo * I->S, (size_t)(G ? G->P : I->P) * (size_t)I->S, &warn);
    });
    if (rc < 0) return rc;
  }
  if (outNumericalWarning) *outNumericalWarning = warn;
  return PHYHIP_SUCCESS;
}

int phyhip_profile_read_node_posteriors(int instance, double *outKernelMs, int *outCalls)
{
  double ms = 0.0;
  int    n = 0;
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long, long long) {
    auto &U = side_of(I).anc;
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
