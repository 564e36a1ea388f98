// phyhip_side.hpp -- the host layer of the units beside the hot path (phyhip_exact.hip, phyhip_ancestral.hip, phyhip_dist.hip,
// phyhip_support.hip, phyhip_pars.hip, phyhip_brlen.hip, phyhip_regraft.hip, phyhip_triple.hip): a work space grown on use, the walk over the plain instance or every shard, the refusals
// by kind of instance, the kernel timer of a profiled instance, and what those units keep on the instance.  Host code only.
// The calls that run a list of candidates in chunks take their work-space layouts from phyhip_scan_plan.hpp and their chunk loop
// from phyhip_scan.hpp.
#pragma once
#include "phyhip_host.hpp"
#include "phyhip_scan_plan.hpp"

#pragma GCC visibility push(hidden) // (inline functions of this header stay out of the library's dynamic symbols)
namespace phyhip_host
{

// ---- work space ------------------------------------------------------------------------------------------------------------------
// hipMalloc with the side calls' report; *ptr is nullptr afterwards where it failed
inline int side_alloc(void **ptr, size_t bytes, const char *who)
{
  const hipError_t e = hipMalloc(ptr, bytes);
  if (e == hipSuccess) return 0;
  (void)hipGetLastError();
  *ptr = nullptr;
  return fail(e == hipErrorOutOfMemory ? PHYHIP_ERROR_OUT_OF_MEMORY : PHYHIP_ERROR_GENERAL, "%s: %zu bytes of work space: %s", who, bytes,
              hipGetErrorString(e));
}

// device memory allocated or grown on use and kept on the instance
struct WorkSpace
{
  void  *ptr = nullptr;
  size_t cap = 0;
  bool   holds(size_t bytes) const { return ptr && cap >= bytes; } // (false: reserve() will free and allocate)
  template <class T> T *at(size_t byte_offset) const { return reinterpret_cast<T *>(static_cast<char *>(ptr) + byte_offset); }
  // grow-only; what it held is NOT kept.  Empty afterwards where the allocation failed.
  int reserve(size_t bytes, const char *who)
  {
    if (holds(bytes)) return 0;
    release();
    if (const int rc = side_alloc(&ptr, bytes, who)) return rc;
    cap = bytes;
    return 0;
  }
  void release()
  {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
};

// ---- refusals that belong to the kind of instance ---------------------------------------------------------------------------------
enum : unsigned { kRefuseRank = 1, kRefuseClassAxis = 2, kRefuseGenericLoop = 4, kRefuseStates = 8 };
inline int refuse_kind(const Instance *I, const char *who, unsigned what)
{
  const char *kind = (what & kRefuseRank) && I->co                  ? "a rank of phyhip_comm_init_rank (it holds only its own patterns)"
                     : (what & kRefuseClassAxis) && I->class_axis   ? "class-axis instances"
                     : (what & kRefuseGenericLoop) && I->generic_loop ? "generic-loop instances"
                                                                      : nullptr;
  if (kind) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %s", who, kind);
  if ((what & kRefuseStates) && I->S != 4 && I->S != 20) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "%s: not built for %d states", who, I->S);
  return 0;
}

// ---- the plain instance, or each shard of a one-process sharded one in pattern order ---------------------------------------------
// How the group is looked up: draining the queue-only likelihood calls it has recorded (a replay that failed is returned before any
// shard is entered), or leaving them recorded.  How each instance is entered: as a call that may put work on its stream (the
// large-grid resident workgroups leave), or as a query that keeps them and leaves the stream's state as it was found.
enum SideLookup { kSideDrain, kSideNoDrain };
enum SideEntry { kSideCall, kSideQuery };

template <bool Query, typename F> int side_one(int id, long long lo, long long n, F &f)
{
  GET_INST_AS(I, id, Query);
  const int rc = f(I, lo, n < 0 ? I->P : n);
  if constexpr (Query) I_call.leave_query();
  return rc;
}

// f(Instance *, first pattern, pattern count) inside one Entered<> object per instance
template <SideLookup L, SideEntry E, typename F> int side_each(int instance, F &&f)
{
  Group *G = L == kSideDrain ? get_group(instance) : get_group_nodrain(instance);
  if (!G) return side_one<E == kSideQuery>(instance, 0, -1, f);
  if (L == kSideDrain)
    if (const int rc = group_take_drain_error(G)) return rc;
  for (size_t g = 0; g < G->sub_id.size(); ++g)
  {
    const int rc = side_one<E == kSideQuery>(G->sub_id[g], G->lo[g], G->n[g], f);
    if (rc < 0) return rc;
  }
  return PHYHIP_SUCCESS;
}

// the instances of a call that works on all of them at once (the Entered<> objects are gone when it does), none of a refused kind
struct SideShards
{
  std::vector<Instance *> sh;
  std::vector<long long>  lo; // first pattern of each
  long long               P = 0; // patterns of the whole
};
inline int side_collect(int instance, const char *who, unsigned refuse, SideShards &s)
{
  const int rc = side_each<kSideDrain, kSideCall>(instance, [&](Instance *I, long long lo, long long n) {
    s.sh.push_back(I);
    s.lo.push_back(lo);
    s.P += n;
    return 0;
  });
  if (rc < 0) return rc;
  if (s.sh.empty()) return fail(PHYHIP_ERROR_GENERAL, "%s: an instance without shards", who);
  for (const Instance *X : s.sh)
    if (const int r = refuse_kind(X, who, refuse)) return r;
  return PHYHIP_SUCCESS;
}

// ---- HIP events around a unit's kernels while the instance is being profiled -----------------------------------------------------
// Made by the first tic() and only while I->prof; destroyed on every way out unless handed on (detach)
struct SideTimer
{
  const bool        on;
  const hipStream_t stream;
  hipEvent_t        e[2] = {nullptr, nullptr};
  bool              marked = false;
  explicit SideTimer(const Instance *I) : on(I->prof), stream(I->stream) {}
  SideTimer(const SideTimer &) = delete;
  ~SideTimer()
  {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int tic()
  {
    if (!on) return 0;
    for (hipEvent_t &x : e)
      if (!x) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(e[0], stream));
    marked = false;
    return 0;
  }
  int mark() // the end of the interval, nothing waited for
  {
    if (on && !marked) HIPCHK(hipEventRecord(e[1], stream));
    marked = true;
    return 0;
  }
  // the interval since tic() added to ms_sum, once the stream has reached its end (marked here unless mark() did)
  int toc(double &ms_sum)
  {
    if (!on) return 0;
    float ms = 0.0f;
    if (const int rc = mark()) return rc;
    HIPCHK(hipEventSynchronize(e[1]));
    HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
    ms_sum += (double)ms;
    return 0;
  }
  std::pair<hipEvent_t, hipEvent_t> detach() // the pair is the caller's from here
  {
    const std::pair<hipEvent_t, hipEvent_t> p(e[0], e[1]);
    e[0] = e[1] = nullptr;
    return p;
  }
};

// ---- what the units keep on the instance (Instance::side, made on first use) ------------------------------------------------------
constexpr size_t kDistBandBytes = 128u << 20; // pairwise distances: the raw counts of one band of taxa stay below this by default
constexpr size_t kRegraftWorkBytes = kDistBandBytes; // regraft scans (plain and mixture): the work space stays below this by default (a longer list runs in chunks)

// a regraft scan, plain or mixture
struct RegraftUnit
{
  WorkSpace  work;                          // as `lay` places it
  ScanLayout lay;                           // of the last call (phyhip_scan_plan.hpp): the getters read through it
  size_t     max_bytes = kRegraftWorkBytes; // the bound on the work space (phyhip_set_regraft_work_space, phyhip_set_mixture_regraft_work_space)
  bool       valid = false;                 // a call has completed: the getters may read what it left
  int        classes = 0;                   // of the last call: its classes (mixture), ...
  int        chunks = 0, last_first = 0;    // ... its chunks, the first candidate of the last one
  int        last_count = 0, last_keep = -1;
  std::vector<int> last_slots;              // ... [candidate of the last chunk][3]: the matrix slots its record named
  double     prof_ms = 0.0;                 // while profiling: its kernels (phyhip_profile_read_regraft, phyhip_profile_read_mixture_regraft)
  int        prof_n = 0;
  long long  prof_cand = 0;                 // ... and the candidates they served
};

struct SideUnits
{
  struct
  {
    WorkSpace out; // outputs of phyhip_calculate_edge_site_outputs_exact
  } exact;
  struct
  {
    WorkSpace work;          // phyhip_calculate_node_state_posteriors
    double    prof_ms = 0.0; // while profiling: its kernel launches (phyhip_profile_read_node_posteriors)
    int       prof_n = 0;
  } anc;
  struct
  {
    WorkSpace work;                        // phyhip_calculate_pairwise_ml_distances
    size_t    band_bytes = kDistBandBytes; // the bound on the raw counts held at a time (phyhip_set_pairwise_work_space)
    double    prof_count_ms = 0.0, prof_opt_ms = 0.0; // while profiling: its count / optimise kernels (phyhip_profile_read_pairwise)
    int       prof_n = 0;
  } dist;
  struct
  { // phyhip_calculate_sh_support; all of it lives on the first shard of a sharded instance
    WorkSpace slots; // the three per-pattern vectors log_lks_aLRT[0..2], [3][P of the whole instance]
    bool      slot_set[3] = {false, false, false};
    WorkSpace work;  // weights, alias table, gather table, sums and flags
    unsigned long long epoch = 0; // Instance::wght_epoch summed over the shards when the alias table was built
    int       sites = 0;          // ... and the site count it was built for
    bool      alias_valid = false, table_on_device = false; // the host's table is current; `work` holds it
    long long dev_P = 0;
    std::vector<double> w, prob; // the weights the table was built from (all shards) and Sample_n_i_With_Proba_pi's prob
    std::vector<int>    alias;   // ... and alias
    double    prof_ms = 0.0;     // while profiling: its kernels (phyhip_profile_read_support)
    int       prof_n = 0;
  } sup;
  struct
  { // phyhip_optimise_edge_length
    void     *h_out = nullptr; // host-mapped: the record the search kernel writes (phyhip_brlen.hip, BrlenResult)
    double    prof_ms = 0.0;   // while profiling: its kernel (phyhip_profile_read_edge_length)
    int       prof_n = 0;
    long long prof_evals = 0;  // ... and the evaluations its searches took
  } brlen;
  RegraftUnit regraft;    // phyhip_calculate_regraft_log_likelihoods (classes stays 0)
  RegraftUnit mixregraft; // phyhip_calculate_mixture_regraft_log_likelihoods; all of it lives on the FIRST class instance (of each shard)
  struct
  { // phyhip_optimise_triples
    WorkSpace work;                          // as `lay` places it
    TripleLayout lay;                        // of the last call (phyhip_scan_plan.hpp)
    size_t    max_bytes = kRegraftWorkBytes; // the bound on it (phyhip_set_triple_work_space)
    bool      keep_valid = false;            // the last call kept a candidate that ran to its end: phyhip_get_triple_partials may read it
    double    prof_ms = 0.0;                 // while profiling: its kernel (phyhip_profile_read_triples)
    int       prof_n = 0;
    long long prof_evals = 0;                // ... and the evaluations its searches took
  } triple;
};

inline SideUnits &side_of(Instance *I)
{
  if (!I->side) I->side = new SideUnits;
  return *I->side;
}

// A side call has waited for the instance's stream and nothing queued is left: clean at once, as after a fenced evaluation
// (phyhip_queue.hip) -- the Lk(b) / dLk calls that follow can be served resident again
inline void side_stream_drained(Instance *I)
{
  I->stream_dirty = false; I->clean_after = 0; ++I->clean_epoch;
}

inline void side_release(Instance *I) // phyhip_finalize_instance
{
  if (!I->side) return;
  for (WorkSpace *w : {&I->side->exact.out, &I->side->anc.work, &I->side->dist.work, &I->side->sup.slots, &I->side->sup.work, &I->side->regraft.work,
                       &I->side->mixregraft.work, &I->side->triple.work})
    w->release();
  if (I->side->brlen.h_out) (void)hipHostFree(I->side->brlen.h_out);
  delete I->side;
  I->side = nullptr;
}

} // namespace phyhip_host
#pragma GCC visibility pop
