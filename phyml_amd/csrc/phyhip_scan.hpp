// phyhip_scan.hpp -- the host driver of the calls that take a list of K candidates and run it in chunks under a work-space bound:
// the checks and the devirtualising of a regraft candidate list, the reservation of a scan's work space, the chunk walk, and the
// chunk loop of the two regraft scans (phyhip_regraft.hip) -- pack, one copy up, launch, wait, one copy down, bookkeeping.  A unit
// brings its refusals, its kernel parameters and a callable that launches its kernels.  Host code only; the layouts: phyhip_scan_plan.hpp.
#pragma once
#include "phyhip_side.hpp"

#pragma GCC visibility push(hidden) // (inline functions of this header stay out of the library's dynamic symbols)
namespace phyhip_host
{

// every record names buffers or tips of I, and no tip as the left operand
inline int regraft_check_candidates(const Instance *I, const phyhip_regraft_candidate *cand, int count, const char *who)
{
  int rc;
  for (int k = 0; k < count; ++k)
  {
    const phyhip_regraft_candidate &c = cand[k];
    if ((rc = check_partial_index(I, c.child1Partials, true)) || (rc = check_partial_index(I, c.child2Partials, true)) ||
        (rc = check_partial_index(I, c.subtreePartials, true)))
      return fail(rc, "%s: candidate %d: %s", who, k, std::string(g_err).c_str());
    if ((c.flags & PHYHIP_REGRAFT_SUBTREE_IS_LEFT) && c.subtreePartials < I->tips)
      return fail(PHYHIP_ERROR_OUT_OF_RANGE, "%s: candidate %d: tip %d as the left operand", who, k, c.subtreePartials);
  }
  return 0;
}

// the buffers the records name stored, queued matrix work and partial updates run (the path updates of the caller are seen), the
// stream drained, the tip masks on the device
inline int regraft_make_real(Instance *I, const phyhip_regraft_candidate *cand, int count)
{
  for (int k = 0; k < count; ++k)
    for (const int buf : {cand[k].child1Partials, cand[k].child2Partials, cand[k].subtreePartials}) devirtualise(I, buf);
  if (const int rc = flush_sync(I)) return rc;
  return upload_masks(I);
}

// the call's layout under the unit's bound, left on the unit, and its work space
inline int scan_reserve(RegraftUnit &U, const Instance *I, int matrices_per_slot, int classes, int count, const char *who)
{
  const ScanLayout size(I->P, I->S, matrices_per_slot, classes, 0);
  U.lay = ScanLayout(I->P, I->S, matrices_per_slot, classes, scan_chunk(U.max_bytes, size.fixed, size.per, count, kScanGridCap));
  return U.work.reserve(U.lay.total, who);
}

// body(first, n, keep_cand) for every chunk in list order; keep_cand: the kept candidate as the chunk counts, or -1
template <class Body> int for_each_chunk(int count, size_t chunk, int keep, Body &&body)
{
  for (size_t first = 0; first < (size_t)count; first += chunk)
  {
    const size_t n = std::min(chunk, (size_t)count - first);
    const int    keep_cand = (keep >= (int)first && keep < (int)(first + n)) ? keep - (int)first : -1;
    if (const int rc = body(first, n, keep_cand)) return rc;
  }
  return 0;
}

// body() queues a chunk's kernels on I's stream; they are timed while I is profiled, and waited for
template <class Body> int side_timed(SideTimer &tm, Instance *I, double &prof_ms, Body &&body)
{
  int rc;
  if ((rc = tm.tic())) return rc;
  if ((rc = body())) return rc;
  HIPCHK(hipGetLastError());
  if ((rc = tm.mark())) return rc;
  HIPCHK(hipStreamSynchronize(I->stream));
  return tm.toc(prof_ms);
}

// The chunk loop of a regraft scan on I's stream, in the work space scan_reserve() left on U.  prefix: what goes up in front of the
// records (U.lay.prefix_bytes of it: the mixture's head and class table), or NULL.
// launch(n, n_lengths, keep_cand, d_recs, d_lengths, d_flags, d_out) queues the unit's matrix kernel (which zeroes the n flags), its
// scan kernel and regraft_sum_kernel for a chunk of n candidates that name n_lengths distinct lengths, and returns 0 or an error.
template <class Launch>
int scan_chunks(RegraftUnit &U, Instance *I, const phyhip_regraft_candidate *cand, int count, int keep, double *sums, int *warns, const void *prefix,
                Launch &&launch)
{
  const ScanLayout       &L = U.lay;
  std::vector<RegraftRec> recs;
  SlotTable               slots;
  std::vector<char>       up;
  std::vector<double>     down;
  SideTimer               tm(I);
  U.chunks = 0;
  const int rc = for_each_chunk(count, L.chunk, keep, [&](size_t first, size_t n, int keep_cand) {
    recs.clear();
    slots.reset();
    for (size_t k = 0; k < n; ++k) recs.push_back(regraft_pack(cand[first + k], slots));
    const size_t n_len = slots.lengths.size();
    up.resize(L.prefix_bytes + n * sizeof(RegraftRec) + n_len * sizeof(double));
    if (prefix) memcpy(up.data(), prefix, L.prefix_bytes);
    memcpy(up.data() + L.prefix_bytes, recs.data(), n * sizeof(RegraftRec));
    memcpy(up.data() + L.prefix_bytes + n * sizeof(RegraftRec), slots.lengths.data(), n_len * sizeof(double));
    HIPCHK(hipMemcpyAsync(U.work.at<char>(L.prefix), up.data(), up.size(), hipMemcpyHostToDevice, I->stream));
    double *const d_down = U.work.at<double>(L.flags(n)); // (where the scan kernel of a launch of n candidates looks for its flags)
    const RegraftRec *d_recs = U.work.at<const RegraftRec>(L.recs);
    const double     *d_lengths = U.work.at<const double>(L.lengths(n));
    if (const int r = side_timed(tm, I, U.prof_ms, [&] { return launch(n, n_len, keep_cand, d_recs, d_lengths, (int *)d_down, U.work.at<double>(L.sums(n))); }))
      return r;
    down.resize(2 * n);
    HIPCHK(hipMemcpy(down.data(), d_down, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
    memcpy(sums + first, down.data() + n, n * sizeof(double));
    for (size_t k = 0; k < n; ++k) warns[first + k] = reinterpret_cast<const int *>(down.data())[k] ? 1 : 0;
    ++U.chunks;
    U.last_first = (int)first;
    return 0;
  });
  if (rc) return rc;
  // the last chunk's matrices stay in the work space for the transition-matrix getter
  U.last_slots.clear();
  for (const RegraftRec &r : recs) U.last_slots.insert(U.last_slots.end(), {r.m1, r.m2, r.m3});
  U.last_count = count; U.last_keep = keep; U.valid = true;
  if (I->prof) ++U.prof_n, U.prof_cand += count;
  return 0;
}

} // namespace phyhip_host
#pragma GCC visibility pop
