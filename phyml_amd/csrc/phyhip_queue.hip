// phyhip_queue.hip -- the deferred operation queue turned into launches, and the waits for their scalars
// (libphyhip.so, gfx950 only; the units and what they share: phyhip_host.hpp)
#include "phyhip_host.hpp"
#include <algorithm>

namespace phyhip_host
{

// Host-computed matrices queued by phyhip_set_transition_matrix: one launch per kUploadBatch of them.
int flush_uploads(Instance *I)
{
  const auto &up = I->uploads;
  if (!up.empty())
  { // (the upload kernel writes the matrix table: behind the exit of the large-grid resident workgroups, whose own rebuilt
    // matrices sit in their L2s until they leave -- reachable from entry points that keep them, phyhip.hip)
    big_release(I);
    I->touched_call = true;
  }
  size_t done = 0;
  while (done < up.size())
  {
    const int n = (int)std::min<size_t>(up.size() - done, kUploadBatch);
    MatUploadParams q;
    memset(&q, 0, sizeof q);
    q.count = n; q.S = I->S; q.C = I->C; q.pmats = I->d_pmats; q.afrag = I->perm ? I->d_afrag : nullptr;
    for (int k = 0; k < kUploadBatch; ++k) q.shadow[k] = -1;
    for (int k = 0; k < n; ++k) { q.idx[k] = up.idx()[done + k]; q.src[k] = up.payload()[done + k]; q.shadow[k] = up.snapshot()[done + k]; }
    hipLaunchKernelGGL(upload_matrices_kernel, dim3(n), dim3(256), q.afrag ? sizeof(double) * (size_t)I->C * I->S * I->S : 0, I->stream, q);
    HIPCHK(hipGetLastError());
    done += n;
  }
  I->uploads.clear();
  return 0;
}

// Rebuild every queued transition matrix on the device: one staged copy of (index, length) pairs, one launch.
int flush_pmats(Instance *I)
{
  big_release(I);
  I->touched_call = true;
  int done = 0, rc = 0;
  if (!I->uploads.empty() && (rc = flush_uploads(I))) return rc;
  const auto &pm = I->rebuilds;
  const int   count = (int)pm.size();
  while (done < count)
  {
    const int  n     = std::min(count - done, I->pm_scratch_cap);
    const bool small = n <= kSmallPm; // short lists (SPR: 3 per candidate) ride in the kernel arguments
    PmatParams q;
    memset(&q, 0, sizeof q);
    if (small)
    {
      for (int k = 0; k < kSmallPm; ++k) q.small_shadow[k] = -1;
      for (int k = 0; k < n; ++k)
      {
        q.small_idx[k] = pm.idx()[done + k];
        q.small_len[k] = pm.payload()[done + k];
        q.small_shadow[k] = pm.snapshot()[done + k];
      }
    }
    else
    {
      void        *st = nullptr;
      const bool   sh = pm.snapshots() > 0; // (snapshots of old values for virtual buffers: a third array)
      const size_t bi = (sizeof(int) * n + 15) & ~size_t(15), bl = sizeof(double) * n;
      rc = I->ring.alloc(bi + bl + (sh ? bi : 0), I->stream, &st);
      if (rc) return rc;
      memcpy(st, pm.idx().data() + done, sizeof(int) * n);
      memcpy((char *)st + bi, pm.payload().data() + done, bl);
      if (sh) memcpy((char *)st + bi + bl, pm.snapshot().data() + done, sizeof(int) * n);
      if (I->pm_copy)
      {
        HIPCHK(hipMemcpyAsync(I->d_pmscratch, st, bi + bl, hipMemcpyHostToDevice, I->stream));
        q.indices = (const int *)I->d_pmscratch;
        q.lengths = (const double *)((char *)I->d_pmscratch + bi);
      }
      else
      { // the kernels read the (index, length) pairs straight from the pinned staging chunk: a few hundred bytes over
        // the host link cost less than a copy command ahead of the launch
        q.indices = (const int *)st;
        q.lengths = (const double *)((char *)st + bi);
      }
      if (sh) q.shadow = (const int *)((char *)st + bi + bl); // (always read from the staging chunk)
    }
    q.count = n;
    q.S = I->S; q.C = I->C; q.U = I->d_evec; q.V = I->d_ivec; q.R = I->d_eval; q.rates = I->d_catr;
    q.br_len_mult = I->br_len_mult; q.l_min = I->l_min; q.l_max = I->l_max; q.pmats = I->d_pmats;
    // (20 states: a short list is latency -- 1024 threads, two entries each, products pre-formed: 7.9 vs 11.5 us for three
    // matrices; a whole tree's 397 matrices: 512 threads without the extra phase 14.7 us; 256 / 1024 threads 16.3-17.4 / 15.5)
    int threads = (I->S == 4) ? 64 : (n <= 16 ? 1024 : 512);
    if (const char *e = diag_env("PHYHIP_PMAT_THREADS"))
    { // (a multiple of 64 within the kernel's launch bounds, or ignored)
      const int v = atoi(e);
      if (v >= 64 && v % 64 == 0 && v <= (I->S == 4 ? 64 : 1024)) threads = v;
    }
    q.afrag = I->perm ? I->d_afrag : nullptr; // 20 states: the MFMA A-operand fragments come out of the same kernel
    q.class_axis = I->class_axis ? 1 : 0;
    const size_t lds = sizeof(double) * ((size_t)2 * I->C * I->S + (size_t)2 * I->C * I->S * I->S + (size_t)2 * I->NE * I->S * I->S);
    // 20 states: the register-blocked kernel (phyhip_kernels.hpp: pmat20_kernel).  PHYHIP_PMAT20 (diag) = 0: the LDS-staged
    // pmat_kernel<20> builds every list, 1: it builds the lists of more than 16 matrices
    static const int pmat20 = diag_env("PHYHIP_PMAT20") ? atoi(diag_env("PHYHIP_PMAT20")) : 2;
    if (I->S == 4) hipLaunchKernelGGL((pmat_kernel<4, true>), dim3(n), dim3(threads), lds, I->stream, q);
    else if (pmat20 == 2 || (pmat20 == 1 && n <= 16))
      hipLaunchKernelGGL(pmat20_kernel, dim3(n), dim3(256), sizeof(double) * ((size_t)I->C * 20 + (size_t)2 * I->NE * 400 + (q.afrag ? kAaMat : 0)),
                         I->stream, q);
    else if (n <= 16) hipLaunchKernelGGL((pmat_kernel<20, true>), dim3(n), dim3(threads), lds, I->stream, q);
    else hipLaunchKernelGGL((pmat_kernel<20, false>), dim3(n), dim3(threads), lds, I->stream, q);
    HIPCHK(hipGetLastError());
    done += n;
  }
  I->rebuilds.clear();
  return 0;
}

// Final sum inside the producing kernel (last workgroup) or as a separate 1-block kernel?  Measured on MI355X (round 2,
// docs/history/tools/gpu_step_ab.sh, with PHYHIP_SPLIT_REDUCE actually honoured): fused saves the second launch (~3.4 us + gap)
// whenever the grid is small -- every SPR / Br_Len_Opt call on small and mid-sized alignments.  On large grids it costs
// the traversal kernel ~6-10 % (cfg2 198 vs 186 us, 125 000 patterns 469 vs 414, 1 M 3.54 vs 3.22 ms, cfg3 574 vs 553):
// a workgroup must see its block sum acknowledged by memory before it draws its ticket, i.e. it waits for ALL its
// outstanding result stores instead of retiring behind them, and holds its wave slot meanwhile.  PHYHIP_SPLIT_REDUCE=0/1
// forces either.
bool fuse_reduce(const Instance *I, int nblocks)
{
  if (I->split_reduce_forced) return !I->split_reduce;
  return nblocks <= 512;
}

// ---- flush_impl and its stages -----------------------------------------------------------------------------------------------
// What the stages share besides the kernel arguments (TreeParams q) they fill: the route the call takes, and what the launch has
// to know about the records that were built for it.
namespace
{
struct FlushPlan
{
  int n_queued = 0, n_ops = 0; // operations the caller queued (the unit of phyhip_profile_read's update count); as rewrite_pending left them
  // the route (plan_route)
  bool up_ride = false; // host-computed matrices travel with the evaluation (a launch: TreeParams::n_up; a resident command: ResidentCtl::up_area)
  bool fold_pm = false; // queued device-built matrices are rebuilt by the evaluation itself (TreeParams::n_fresh)
  bool aa_take = false; // the 20-state resident workgroups take the evaluation
  bool big_fit = false, big_try = false, big_take = false; // the large-grid ones may serve it; the stream lets them; they are there
  bool one_shot = false; // ... or they are not, and their kernel is launched for this one evaluation (BigArgs::n_one_shot)
  bool big_cmd() const { return big_take || one_shot; } // (records for that kernel: no forwarding between two operations)
  // the operation records (place_op_records, build_op_records)
  bool             fat = false, has_inl = false; // record pairs of the pipelined kernels, not DevOps; some operation computes a virtual child in its own step
  RegWindow        window{0};                    // how far back the launch's kernel forwards results in registers (reg_window)
  StepPlan         plan_short[2];                // the step plan of a launch of one or two records; a longer one: Instance::step_plan
  const StepPlan  *plan = nullptr;               // ... once somebody asked for it (step_plan)
  bool             compact = false;              // compact records (NtIssue / NtExec), not descriptors
  int              slot_hit = -1;                // the device slot that still holds this very list, or -1
  bool             in_args = false;              // one or two operations of the pipelined kernels, in the kernel arguments
  std::vector<int> aa_slot, aa_need;             // the 20-state LDS ring, per item (plan_aa_ring)
  const IssueRec  *d_irec = nullptr;             // ... in a device slot (nullptr: in the kernel arguments)
  const ExecRec   *d_xrec = nullptr;
  RO               ro;                           // ... or slim DevOps (RO::ops), and the tables every kernel reads
  // the launch
  bool mixed = false;     // a list-form launch of an instance with two wave shapes: traverse_nt2_mixed_kernel's grid, one record per workgroup
  bool bodied = false;    // ... or of any kernel that carries the straight-line step bodies: its compact records name step kinds
  int  soa_grid = 0;      // workgroups of the lane-per-pattern kernel in this launch
  int  host_sum_n = 0;    // > 0: the host adds this many posted records (Instance::host_sum_n)
  bool fused_sum = false; // the traversal kernel's last workgroup finishes the sum
};

// What a launcher returns when it found no instantiation for this instance: the next kernel family is tried.  It shares the
// int with the launchers' error codes, which are all negative (PHYHIP_ERROR_*), and with 0 for "launched".
constexpr int kNotLaunched = 1;
} // namespace

// ... in a resident command: where the host stores into device memory (a pushed record)
static bool up_resident(const Instance *I, const FlushPlan &f, const Resident &R) { return f.up_ride && I->push_cmds != 0 && (R.cmd ? R.pushed && R.up_area != nullptr : true); }

// Resident workgroups are not ordered with the stream: is everything on it known to be finished?  Waits (bounded: 200 us, else
// the ordinary launch) for the report of the last Update_Eigen_Lr.
static bool stream_clean_for_resident(Instance *I)
{
  bool clean = !I->dirty_prev && !I->touched_call;
  if (clean && I->clean_after)
  {
    volatile unsigned long long *stamp = reinterpret_cast<volatile unsigned long long *>(I->h_result + 3);
    struct timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long it = 1; *stamp < I->clean_after && clean; ++it)
    {
      __builtin_ia32_pause();
      if ((it & 255) == 0 && ns_since(t0) > 200000.0) clean = false;
    }
    if (clean) { __atomic_thread_fence(__ATOMIC_ACQUIRE); I->clean_after = 0; ++I->clean_epoch; }
  }
  if (!clean) ++I->rt.n_busy;
  return clean;
}

// The queue is in the stream (or in a resident command): forget it.  Matrix rebuilds that rode with the evaluation go with it.
static void retire_queue(Instance *I, bool fold_pm)
{
  // (no snapshot is lost with them: plan_route sets fold_pm only where rebuilds.snapshots() == 0 -- the aa_take condition and the
  // nucleotide condition both say so)
  if (fold_pm) I->rebuilds.clear();
  I->pending.clear();
  I->unstored.n_front = 0;
  clear_matrix_readers(I);
}

// Which of the five routes takes the call: an ordinary launch, the short-launch resident evaluator (decided later, once the
// records say whether it can: try_resident_nt2), the 20-state resident evaluator, the large-grid one, or that kernel launched
// one-shot -- and whether the queued matrices travel with it.  (< 0: the large-grid workgroups could not be launched)
static int plan_route(Instance *I, const EdgeEval *ee, FlushPlan &f)
{
  const int n_ops = f.n_ops;
  // a short list of device-built matrices is folded into the lane-per-pattern nucleotide kernel's prologue when the grid
  // is small (measured: 16.7 vs 17.8 us per scalar-returning call on a 382-pattern search prefix; at 100 000 patterns
  // the redundant per-workgroup rebuild costs more than the launch it saves: 45.1 vs 42.5 us per SPR candidate)
  static const int fold_grid_max = diag_env("PHYHIP_FOLD_GRID") ? atoi(diag_env("PHYHIP_FOLD_GRID")) : 512;
  // a short list of HOST-computed matrices rides in the arguments of the lane-per-pattern nucleotide kernel at every grid size
  // (TreeParams::n_up): no upload kernel in front of the traversal
  f.up_ride = I->soa && I->arg_uploads && !I->uploads.empty() && (int)I->uploads.size() <= kArgUp && I->rebuilds.empty() &&
              (n_ops > 0 || ee) && I->C <= 4 && !I->class_axis && !(I->ablate & 8) && I->uploads.snapshots() == 0;
  // large grids: an evaluation the large-grid resident workgroups can take (phyhip_big.hpp) carries its matrices in the command
  // (host-computed matrices -- the bit-exact route -- stay with the one-wave launch that takes them in its arguments: the
  // large-grid kernel launched with them in ITS arguments was measured, 30-31 against 28.4 us per candidate at 500 x 100 000)
  const bool big_form0 = ee && (ee->eigen || (ee->to_host && !ee->dev_out)) && n_ops <= 2 && I->args_recs && I->fold_pmats &&
                         (int)I->rebuilds.size() <= 4 && !I->rt_skip; // (an evaluation that kernel can take)
  const bool big_form = big_form0 && I->uploads.empty();
  f.big_fit = big_form0 && (I->uploads.empty() || up_resident(I, f, I->rb)) && big_eligible(I) && !I->prof;
  f.big_try = f.big_fit && big_ready(I);
  // ... and they are there (or launched now): decided before the records are built -- a resident command of two operations runs
  // them one after the other per tile, without register forwarding between them (phyhip_big.hpp)
  if (f.big_try)
  {
    const int brc = big_ensure(I);
    if (brc < 0) return brc;
    f.big_take = brc == 0 && (I->uploads.empty() || up_resident(I, f, I->rb)); // (a record that turned out to live in host memory: launch)
  }
  // ... or they are not, and the same kernel is LAUNCHED for this one evaluation (BigArgs::n_one_shot) instead of pmat_kernel +
  // a traversal of one-wave workgroups + a record per workgroup: where the final sum can run through one partial sum per
  // workgroup (256 workgroups, more tiles than the host adds itself)
  f.one_shot = big_form && !f.big_take && I->big_oneshot && big_shape(I) && I->spin_wait && I->dev >= 0 && I->grid_nt2 > I->big_device_sum &&
               big_sum_by_group(I, I->grid_nt2);
  if (kDiag && ee && getenv("PHYHIP_RESIDENT_DEBUG") && big_shape(I))
    fprintf(stderr, "big: fit %d try %d | eligible %d ops %d pm %zu up %zu prof %d skip %d | dirty_prev %d touched %d clean_after %llu stamp %llu streak %d launched %d owner %p me %p\n",
            (int)f.big_fit, (int)f.big_try, (int)big_eligible(I), n_ops, I->rebuilds.size(), I->uploads.size(), (int)I->prof, (int)I->rt_skip, (int)I->dirty_prev,
            (int)I->touched_call, I->clean_after, *reinterpret_cast<volatile unsigned long long *>(I->h_result + 3), I->big_streak, (int)I->rb.launched,
            (void *)g_big_owner[I->dev < 64 ? I->dev : 0].load(), (void *)I);
  // small 20-state alignments: an evaluation the resident workgroups of traverse_aa_kernel<..., RES> can take -- decided here, before
  // the matrix queue is dealt with, because they rebuild the queued matrices themselves (a launched 20-state kernel cannot: without
  // them the rebuild is pmat20_kernel's launch in front)
  if (resident_aa_eligible(I) && ee && !ee->eigen && ee->to_host && !ee->dev_out && n_ops <= 2 && I->args_recs && I->fold_pmats &&
      (int)I->rebuilds.size() <= 4 && I->uploads.empty() && I->rebuilds.snapshots() == 0 && !I->prof && !I->rt_skip)
  {
    // (a rebuilt matrix the command does not read goes through the ring's spare item: two tables)
    int unread = 0;
    for (int m : I->rebuilds.idx())
    {
      bool read = m == ee->pm;
      for (const DevOp &o : I->pending) read = read || o.pm1 == m || o.pm2 == m;
      unread += !read;
    }
    if (unread > 2) ++I->rt.n_busy;
    else f.aa_take = stream_clean_for_resident(I);
  }
  f.fold_pm = (f.aa_take && !I->rebuilds.empty()) ||
              (I->soa && I->fold_pmats && (I->grid_nt2 <= fold_grid_max || f.big_try || f.one_shot) && !I->rebuilds.empty() && (int)I->rebuilds.size() <= 8 &&
               I->uploads.empty() && (n_ops > 0 || ee) && I->C <= 4 && !I->class_axis && !(I->ablate & 8) && I->rebuilds.snapshots() == 0);
  return 0;
}

// The matrices that travel with the evaluation, into the kernel arguments
static void fill_matrix_args(Instance *I, const FlushPlan &f, TreeParams &q)
{
  if (f.up_ride)
  {
    q.n_up = (int)I->uploads.size();
    for (int k = 0; k < q.n_up; ++k)
    {
      q.up_idx[k] = I->uploads.idx()[k];
      memcpy(q.up_val[k], I->uploads.payload()[k], sizeof(double) * 16 * I->C); // (pinned staging memory: an ordinary host read)
    }
    q.pmats_rw = I->d_pmats;
    I->uploads.clear(); // (no snapshot is lost with them: plan_route sets up_ride only where uploads.snapshots() == 0)
  }
  if (f.fold_pm)
  {
    q.n_fresh = (int)I->rebuilds.size();
    for (int k = 0; k < q.n_fresh; ++k) { q.fresh_idx[k] = I->rebuilds.idx()[k]; q.fresh_len[k] = I->rebuilds.payload()[k]; }
    // (4 states, one eigen system, <= 4 categories: see fold_pm) the eigen system rides in the arguments as well
    if (I->S == 4)
    {
      memcpy(q.m_evec, I->h_evec.data(), 16 * sizeof(double)); memcpy(q.m_ivec, I->h_ivec.data(), 16 * sizeof(double));
      memcpy(q.m_eval, I->h_eval.data(), 4 * sizeof(double));
      for (int c = 0; c < 4; ++c) q.m_rates[c] = c < I->C ? I->h_rates[c] : 0.0;
    }
    q.br_len_mult = I->br_len_mult; q.l_min = I->l_min; q.l_max = I->l_max; q.pmats_rw = I->d_pmats;
    // (the matrix queue is cleared only after the launch that rebuilds it has been issued: retire_queue)
  }
}

// 20-state kernel, a list with in-step children: an item of its LDS ring is two matrix tables or -- with an in-step child -- four.
// The host hands out the table slots (8 tables; an item never wraps) and says, per item, how many items every consumer must have
// released before the loader may overwrite them (phyhip_aa.hpp)
static void plan_aa_ring(const Instance *I, const EdgeEval *ee, FlushPlan &f, TreeParams &q)
{
  if (!(I->perm && f.has_inl)) return;
  const int n_ops = f.n_ops, n_rec = n_ops + (n_ops & 1), n_items = n_rec + (ee ? 1 : 0);
  f.aa_slot.resize(n_items); f.aa_need.resize(n_items);
  int cur = 0, owner[2 * kAaRing];
  for (int &x : owner) x = -1;
  for (int k = 0; k < n_items; ++k)
  {
    const int nt = (k < n_rec && (I->pending[std::min(k, n_ops - 1)].pad & (kOpInl1 | kOpInl2))) ? 4 : 2;
    if (cur + nt > 2 * kAaRing) cur = 0;
    int need = 0;
    for (int t = cur; t < cur + nt; ++t) { need = std::max(need, owner[t] + 1); owner[t] = k; }
    f.aa_slot[k] = cur; f.aa_need[k] = need;
    cur = (cur + nt) % (2 * kAaRing);
  }
  if (ee) { q.aa_e_slot = f.aa_slot[n_rec]; q.aa_e_need = f.aa_need[n_rec]; }
}

// The register window of the kernel that runs the records (phyhip_step_plan.hpp): the one place that chooses its depth
static RegWindow reg_window(const Instance *I, bool fat, bool big_cmd) { return RegWindow{(!fat || big_cmd) ? 0 : (I->prefetch_dist == 2 ? 2 : 1)}; }

static Desc make_desc(const void *base, size_t bytes, unsigned x) { return Desc{(unsigned long long)(uintptr_t)base, (unsigned)bytes, x}; }

// One child of an operation into the three descriptors the issue stage reads; returns the operation's flag bits it sets.
// reach: how the child comes to the step (the launch's step plan, phyhip_step_plan.hpp); in_step: the definition of the operation's
// in-step child -- a virtual tip x tip result computed inside its step, and this is how
static unsigned child_descs(const Instance *I, int c, bool second, Reach reach, unsigned pmoff, unsigned matbytes, const InlineDef *in_step,
                            Desc &data, Desc &scale, Desc &tip)
{
  if (reach == Reach::InStep)
  { // (kOpCh1 / kOpCh2, phyhip_kernels.hpp) no load of its own -- its two matrices' offsets, its first tip's row in the auxiliary
    // slot, its second tip's row in the tip slot
    const unsigned long long ab = (unsigned long long)((unsigned)in_step->pmA * matbytes) | ((unsigned long long)((unsigned)in_step->pmB * matbytes) << 32);
    if (I->perm)
    { // (20 states: the operation's two tip slots carry the plan of its ring item and the second tip's mask row -- fill_records)
      data  = make_desc(nullptr, 0, pmoff);
      scale = make_desc(I->d_tipmasks + (size_t)in_step->a * I->Ppad, (size_t)I->Ppad * 4, 1);
    }
    else
    {
      data  = make_desc(reinterpret_cast<const void *>((uintptr_t)ab), 0, pmoff);
      scale = make_desc(I->d_tipcodes + (size_t)in_step->a * I->Ppad, (size_t)I->Ppad, 1);
      tip   = make_desc(I->d_tipcodes + (size_t)in_step->b * I->Ppad, (size_t)I->Ppad, 1);
    }
    return second ? kOpCh2 : kOpCh1;
  }
  const bool   t = reach == Reach::Tip, f1 = reach == Reach::Prev1, f2 = reach == Reach::Prev2;
  const bool   ld = reach == Reach::Loaded && !I->no_loads; // (PHYHIP_NOLOADS zeroes the load; the child's reach stays what it is)
  const size_t b = ld ? (size_t)(c - I->tips) : 0;
  data  = make_desc(I->d_partials + b * buf_elems(I), ld ? buf_elems(I) * sizeof(double) : 0, pmoff);
  scale = make_desc(I->d_scales + b * scale_elems(I), ld ? scale_elems(I) * 4 : 0, 0);
  tip   = make_desc(I->d_tipcodes + (size_t)(t ? c : 0) * I->Ppad, (t && !I->soa) ? (size_t)I->Ppad : 0, 0); // (lane-per-pattern kernel: only an in-step child uses this slot)
  // lane-per-pattern nucleotide kernel and the 20-state kernel: ONE auxiliary dword load per child -- the scale
  // descriptor of a tip child points at its tip row instead (spare word 1: the kernel then reads the aligned dword
  // holding the byte)
  if (I->soa && t) scale = make_desc(I->d_tipcodes + (size_t)c * I->Ppad, (size_t)I->Ppad, 1);
  if (I->perm && t) scale = make_desc(I->d_tipmasks + (size_t)c * I->Ppad, (size_t)I->Ppad * 4, 1); // (the mask itself)
  return (t ? (second ? kOpTip2 : kOpTip1) : 0u) | (f1 ? (second ? kOpF21 : kOpF11) : 0u) | (f2 ? (second ? kOpF22 : kOpF12) : 0u);
}

// One record pair per operation, all address arithmetic done here once.  The kernel alternates two register sets, so an odd
// list is padded with a re-execution of its last operation (idempotent: same inputs, same output, same address) whose
// forwarding flags are those of its own position (the step plan says both).
static void fill_records(const Instance *I, const FlushPlan &f, const StepPlan *plan, IssueRec *ir, ExecRec *xr, int n_rec)
{
  const size_t   bufbytes = buf_elems(I) * sizeof(double);
  // spare word of the data descriptors: byte offset of the child's matrix (natural table, or the MFMA A-fragment table, 20 states)
  const unsigned matbytes = I->perm ? (unsigned)(kAaMat * sizeof(double)) : (unsigned)((size_t)I->C * I->S * I->S * sizeof(double));
  for (int k = 0; k < n_rec; ++k)
  {
    const StepPlan  &p = plan[k];
    const DevOp     &o = I->pending[p.op];
    const InlineDef *inl = (p.reach[0] == Reach::InStep || p.reach[1] == Reach::InStep) ? &I->pending_inl[p.op] : nullptr;
    unsigned         fl = 0;
    fl |= child_descs(I, o.c1, false, p.reach[0], (unsigned)o.pm1 * matbytes, matbytes, inl, ir[k].c1_data, ir[k].c1_scale, ir[k].c1_tip);
    fl |= child_descs(I, o.c2, true, p.reach[1], (unsigned)o.pm2 * matbytes, matbytes, inl, ir[k].c2_data, ir[k].c2_scale, ir[k].c2_tip);
    const size_t b = (size_t)(o.dest - I->tips);
    const bool   st_on = p.stored; // (a result that stays virtual: stores through descriptors of size 0 are dropped)
    xr[k].dst_data  = make_desc(I->d_partials + b * buf_elems(I), st_on ? bufbytes : 0, fl);
    xr[k].dst_scale = make_desc(I->d_scales + b * scale_elems(I), st_on ? scale_elems(I) * 4 : 0, 0);
    if (I->perm && f.has_inl)
    { // the ring item of this operation: first table slot (consumers: dst_scale.x; loader: c2_tip.x), what must be released
      // before it is written (c1_tip.bytes), and -- with an in-step child -- its two tables' offsets and its second tip's masks
      const unsigned long long ab = inl ? ((unsigned long long)((unsigned)inl->pmA * matbytes) | ((unsigned long long)((unsigned)inl->pmB * matbytes) << 32)) : 0ull;
      ir[k].c1_tip = make_desc(reinterpret_cast<const void *>((uintptr_t)ab), (size_t)f.aa_need[k], inl ? (p.reach[0] == Reach::InStep ? 1u : 2u) : 0u);
      ir[k].c2_tip = make_desc(I->d_tipmasks + (size_t)(inl ? inl->b : 0) * I->Ppad, inl ? (size_t)I->Ppad * 4 : 0, (unsigned)f.aa_slot[k]);
      xr[k].dst_scale.x = (unsigned)f.aa_slot[k];
    }
  }
}

// The list form of the lane-per-pattern nucleotide kernel reads compact records (NtIssue / NtExec, phyhip_kernels.hpp): the same
// decisions as fill_records and child_descs -- which loads are live, which row the auxiliary dword comes from, what is forwarded,
// the padded re-execution of an odd list's last operation -- said as flag bits and offsets from the three arenas.
static bool compact_list_form(const Instance *I)
{ // (the shapes launch_soa has an instantiation for; any other falls through to kernels that read descriptors)
  if (!I->soa || I->perm) return false;
  const int g = I->nt_groups;
  return (I->C == 1 && g == 1) || (I->C == 2 && g <= 2) || (I->C == 3 && g == 1) || (I->C == 4 && (g == 1 || g == 2 || g == 4));
}

static int fill_compact_records(Instance *I, const FlushPlan &f, const StepPlan *plan, NtIssue *ir, NtExec *xr, int n_rec)
{
  const size_t data16 = buf_elems(I) * sizeof(double) / 16, scale16 = scale_elems(I) * 4 / 16, tip16 = (size_t)I->Ppad / 16; // (Ppad: a multiple of 64)
  const size_t n_int = (size_t)(I->nbuf - I->tips);
  if (n_int * data16 > 0xffffffffull || (size_t)I->tips * tip16 > 0xffffffffull || I->tips >= (1 << 24))
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "an arena of this instance is beyond the reach of a record's offset (64 GiB, 2^24 tips)");
  const unsigned matbytes = (unsigned)((size_t)I->C * I->S * I->S * sizeof(double));
  long long (&kinds)[2][5] = *reinterpret_cast<long long (*)[2][5]>(I->rec_stats + 2); // (phyhip_get_record_stats: per child, by reach)
  static const int stat_of[5] = {0, 2, 3, 1, 4}; // Reach -> its column there: tip, in-step, forwarded one / two steps, loaded
  auto onehot = [&](int tip) { return (tip_row_bits(I, tip) & 1) != 0; };
  ++I->rec_stats[0];
  for (int k = 0; k < n_rec; ++k)
  {
    const StepPlan  &p = plan[k];
    const DevOp     &o = I->pending[p.op];
    const InlineDef *inl = (p.reach[0] == Reach::InStep || p.reach[1] == Reach::InStep) ? &I->pending_inl[p.op] : nullptr;
    NtIssue          r;
    memset(&r, 0, sizeof r);
    unsigned fl = 0;
    bool     rows_onehot[2] = {false, false}; // for the step's kind: every tip row the child reads is one-hot throughout
    for (int s = 0; s < 2; ++s) // s: 0 child 1, 1 child 2 (the second bit of each pair of flags)
    {
      const int    c = s ? o.c2 : o.c1;
      const size_t b = (size_t)(c - I->tips);
      r.pm[s] = (unsigned)(s ? o.pm2 : o.pm1) * matbytes;
      ++kinds[s][stat_of[(int)p.reach[s]]];
      switch (p.reach[s])
      {
        case Reach::InStep: // its first tip's row as the auxiliary dword, its second tip by index, its two matrices in the data slot and the spare word
          rows_onehot[s] = onehot(inl->a) && onehot(inl->b);
          r.fl |= (kRecIn1 | kRecA1 | kRecT1) << s | (unsigned)inl->b << 8;
          r.data[s] = (unsigned)inl->pmA * matbytes; r.pmx = (unsigned)inl->pmB * matbytes;
          r.aux[s] = (unsigned)((size_t)inl->a * tip16);
          fl |= kOpCh1 << s;
          break;
        case Reach::Tip:
          rows_onehot[s] = onehot(c);
          r.fl |= (kRecA1 | kRecT1) << s; r.aux[s] = (unsigned)((size_t)c * tip16);
          fl |= kOpTip1 << s;
          break;
        case Reach::Prev1: fl |= s ? kOpF21 : kOpF11; break;
        case Reach::Prev2: fl |= s ? kOpF22 : kOpF12; break;
        case Reach::Loaded: // (PHYHIP_NOLOADS zeroes the load; the child's reach stays what it is)
          if (!I->no_loads) { r.fl |= (kRecL1 | kRecA1) << s; r.data[s] = (unsigned)(b * data16); r.aux[s] = (unsigned)(b * scale16); }
          break;
      }
    }
    ir[k] = r;
    // the step's kind, where the kernel this list is launched with carries the straight-line bodies (FlushPlan::bodied); a list
    // of any other kernel is kind 0 throughout
    unsigned kind = kind_of(p, rows_onehot);
    if (!((PHYHIP_NT_KINDS >> kind) & 1) || !f.bodied) kind = 0;
    ++I->step_kinds[k & 1][kind];
    fl |= kind << kRecKindShift;
    const size_t b = (size_t)(o.dest - I->tips);
    xr[k].fl = fl | (p.stored ? kRecStore : 0u);
    xr[k].dst_data = (unsigned)(b * data16); xr[k].dst_scale = (unsigned)(b * scale16); xr[k].pad = 0;
    if (kDiag) { I->last_exec_fl.resize((size_t)n_rec); I->last_exec_fl[(size_t)k] = xr[k].fl; }
  }
  return 0;
}

// (a slot's kind: 0 DevOps, 1 / 2 descriptor records with loads that many operations ahead, 16 + that: compact records.  A
// command for the large-grid resident workgroups reads descriptors)
static int slot_kind_of(const Instance *I, const FlushPlan &f) { return f.fat ? (f.compact ? 16 : 0) + I->prefetch_dist : 0; }

// Where the records will live -- decided on its own, in front of build_op_records, because the launch's form (a list, or records
// in the arguments) decides which kernel runs it, and the kernel what the records may say (FlushPlan::mixed, bodied)
static void place_op_records(const Instance *I, FlushPlan &f)
{
  const int n_ops = f.n_ops;
  if (n_ops == 0) return;
  f.compact = f.fat && compact_list_form(I) && !f.big_cmd();
  const int kind = slot_kind_of(I, f);
  for (int sl = 0; sl < I->ops_slots && f.slot_hit < 0; ++sl)
    if (I->slot_kind[sl] == kind && I->slot_ops[sl].size() == (size_t)n_ops &&
        memcmp(I->slot_ops[sl].data(), I->pending.data(), sizeof(DevOp) * n_ops) == 0 && I->slot_inl[sl] == I->pending_inl)
      f.slot_hit = sl;
  f.in_args = f.slot_hit < 0 && f.fat && (I->soa || I->perm) && I->args_recs && n_ops <= 2;
}

// Which lane-per-pattern kernel a list is launched with, decided once for the records and the launch alike.  fill_compact_records
// used to say `mixed` as mix_n4 > 0 && C == 4 && nt_groups == 2 && !ablate, and flush_impl as the line below, read after
// build_op_records from q.recs_in_args.  Neither was wrong: compact records are built only for a list (n_ops > 0, not in the
// arguments), mix_n4 > 0 only where C == 4 and nt_groups == 2 (phyhip_create_instance), and `bodied` asks for prefetch_dist == 2
// itself -- so the two agreed whenever compact records were built.  (An evaluation alone also travels in the arguments: n_ops == 0.)
static void choose_list_kernel(const Instance *I, FlushPlan &f)
{
  f.mixed    = I->mix_n4 > 0 && f.n_ops > 0 && !f.in_args && I->prefetch_dist == 2 && !I->ablate;
  f.bodied   = I->prefetch_dist == 2 && I->nt_groups >= 2 && (f.mixed || nt2_bodied(I->C, I->nt_groups, f.has_inl));
  f.soa_grid = f.mixed ? I->mix_n2 + I->mix_n4 : I->grid_nt2;
}

// The step plan of this launch (phyhip_step_plan.hpp), made when the first reader asks -- a list found in a device slot is not
// planned again unless its traffic is counted.  Nothing is allocated for one or two records, and a list's plan reuses the
// instance's storage.
static const StepPlan *step_plan(Instance *I, FlushPlan &f)
{
  if (f.plan) return f.plan;
  const int n_rec = padded_records(f.n_ops);
  StepPlan *out = f.plan_short;
  if (n_rec > 2) { I->step_plan.resize((size_t)n_rec); out = I->step_plan.data(); }
  plan_steps(I->pending.data(), f.n_ops, I->pending_inl.empty() ? (const InlineDef *)nullptr : I->pending_inl.data(), I->tips, f.window, kPadBits, n_rec, out);
  return f.plan = out;
}

// The queued operations as the kernel reads them: in a device slot (a list identical to one still sitting there -- repeated
// Lk(NULL) on one topology -- is neither rebuilt nor re-uploaded), or, one or two operations of the pipelined kernels, in the
// kernel arguments (phyhip_nt2.hpp): no staging, no copy command, and the device slots keep the long lists they cache
static int build_op_records(Instance *I, FlushPlan &f, TreeParams &q)
{
  const int  n_ops = f.n_ops;
  const bool fat = f.fat, compact = f.compact, in_args = f.in_args;
  q.last_dest = -1;
  if (n_ops == 0) return 0;
  const int    kind = slot_kind_of(I, f), n_rec = padded_records(n_ops), hit = f.slot_hit;
  const size_t ib = (compact ? sizeof(NtIssue) : sizeof(IssueRec)) * n_rec, xb = (compact ? sizeof(NtExec) : sizeof(ExecRec)) * n_rec;
  int          rc = 0;
  char        *dst = I->d_ops + (size_t)(hit >= 0 ? hit : I->ops_slot) * I->ops_slot_bytes;
  int        new_slot = -1;
  if (hit < 0)
  {
    const size_t bytes = fat ? ib + xb : sizeof(DevOp) * n_ops;
    void        *st = nullptr;
    if (!in_args)
    {
      new_slot = I->ops_slot;
      I->slot_kind[new_slot] = -1; // the slot's old content is gone; it holds the new list only once the copy was issued
      if (bytes > I->ops_slot_bytes)
        return fail(PHYHIP_ERROR_OUT_OF_RANGE, "a launch of %d %s does not fit a device slot of %zu bytes", fat ? n_rec : n_ops,
                    fat ? "operation records" : "operations", I->ops_slot_bytes);
      if ((rc = I->ring.alloc(bytes, I->stream, &st))) return rc;
    }
    if (!fat) memcpy(st, I->pending.data(), bytes);
    else if (compact && !in_args)
    {
      if ((rc = fill_compact_records(I, f, step_plan(I, f), reinterpret_cast<NtIssue *>(st), reinterpret_cast<NtExec *>((char *)st + ib), n_rec))) return rc;
    }
    else fill_records(I, f, step_plan(I, f), in_args ? q.arg_ir : reinterpret_cast<IssueRec *>(st), in_args ? q.arg_xr : reinterpret_cast<ExecRec *>((char *)st + ib), n_rec);
    if (in_args) { q.recs_in_args = 1; q.n_real_ops = n_ops; }
    else HIPCHK(hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, I->stream)); // (reading short lists straight from the pinned staging memory instead was measured: no gain)
  }
  if (hit >= 0 && compact) ++I->rec_stats[1];
  if (!fat) f.ro.ops = reinterpret_cast<const DevOp *>(dst);
  else if (!in_args) { f.d_irec = reinterpret_cast<const IssueRec *>(dst); f.d_xrec = reinterpret_cast<const ExecRec *>(dst + ib); }
  if (fat) q.last_dest = I->pending[n_ops - 1].dest;
  q.n_ops = fat ? n_rec : n_ops;
  if (new_slot >= 0)
  {
    I->slot_ops[new_slot]  = I->pending;
    I->slot_inl[new_slot]  = I->pending_inl;
    I->slot_kind[new_slot] = kind;
    I->ops_slot = (new_slot + 1) % I->ops_slots;
  }
  return 0;
}

// short launch: the kernel fetches the sides of the evaluation edge that no queued operation writes up front
static int edge_prefetch_mask(const Instance *I, const EdgeEval *ee)
{
  auto untouched = [&](int idx) {
    if (idx < I->tips) return false;
    for (const DevOp &o : I->pending)
      if (o.dest == idx) return false;
    return true;
  };
  return (untouched(ee->parent) ? 1 : 0) | (untouched(ee->child) ? 2 : 0);
}

// What follows the queued operations in the same launch: the edge evaluation (and where its sum is finished), or the
// eigen-basis products of Update_Eigen_Lr
static void setup_evaluation(Instance *I, const EdgeEval *ee, FlushPlan &f, TreeParams &q)
{
  const int n_ops = f.n_ops;
  if (ee->eigen)
  { // Update_Eigen_Lr fused behind the queued partial update(s): no sums, the products go to d_dot
    q.edge_eval = 2; q.e_parent = ee->parent; q.e_child = ee->child; q.e_pm = 0; q.dot_out = I->d_dot;
    memcpy(q.m_evec, I->h_evec.data(), 16 * sizeof(double)); memcpy(q.m_ivec, I->h_ivec.data(), 16 * sizeof(double));
    if (n_ops == 0 && I->args_recs) { q.recs_in_args = 1; q.n_real_ops = 0; }
    if (q.recs_in_args) q.e_prefetch = edge_prefetch_mask(I, ee);
    // completion as an evaluation's: every workgroup fences its stores and posts an (empty) record the caller waits for -- the
    // stream is clean when phyhip_update_eigen_lr returns, and the resident workgroups can take the call (the only
    // instances that come here: phyhip_update_eigen_lr)
    q.host_blocks = I->h_blocks; q.host_tag = ++I->seq; q.warn = I->h_warn;
    f.host_sum_n  = f.soa_grid;
    return;
  }
  I->warn_current = false;
  q.edge_eval = 1; q.e_parent = ee->parent; q.e_child = ee->child; q.e_pm = ee->pm;
  if (n_ops == 0 && f.fat && (I->soa || f.aa_take) && I->args_recs) { q.recs_in_args = 1; q.n_real_ops = 0; } // (evaluation-only short launch)
  if (q.recs_in_args) q.e_prefetch = edge_prefetch_mask(I, ee);
  const int nblk = I->soa ? f.soa_grid : (I->perm ? I->grid_aa : (f.fat ? I->grid_nt : I->grid));
  // (fusing on large grids was measured for one-operation launches too: 61.6 vs 41.9 us per SPR candidate at cfg5)
  f.fused_sum = !I->class_axis && fuse_reduce(I, nblk) && !(I->host_sum && ee->to_host && !ee->dev_out);
  if (f.fused_sum)
  { // the traversal kernel's last workgroup finishes the sum and reports to the host
    q.tickets = I->d_tickets; q.result = ee->dev_out ? ee->dev_out : I->d_result;
    q.result_host = ee->to_host ? I->h_result : nullptr; q.warn_host = I->h_warn;
    q.seq = ee->to_host ? ++I->seq : 0ull;
    q.warn_out = ee->warn_out;
  }
  if (!f.fused_sum && ee->to_host && !ee->dev_out && I->host_sum && !I->class_axis)
  { // the workgroups post their sums to the host, which adds them (wait_result) -- at every grid size: on small grids
    // this replaces the ticket draw of the fused sum (block sum written through, atomic, fence, re-read: ~3 us of
    // dependent memory round trips inside a ~10 us kernel), on large ones the second launch
    q.host_blocks = I->h_blocks; q.host_tag = ++I->seq;
    q.warn        = I->h_warn;   // raised straight in host-mapped memory
    *I->h_warn    = 0;
    f.host_sum_n  = nblk;
    if (I->eig_api_no && I->api_no == I->eig_api_no + 1 && (I->soa || I->perm))
    { // (the kernels that honour it; eig_api_no is only set for small alignments with the resident evaluator enabled)
      q.fence_post   = 1;
      I->fenced_eval = true;
    }
  }
  if (I->want_site_outputs) { q.site_lnl = I->d_site_lnl; q.site_lk = I->d_site_lk; q.site_cat = I->d_site_cat; }
}

// ---- resident commands --------------------------------------------------------------------------------------------------------
// The command record of the three resident evaluators that take a traversal's evaluation, as their parsers read it
// (phyhip_nt2.hpp: resident_nt2_kernel; phyhip_aa.hpp: the RES form of traverse_aa_kernel; phyhip_big.hpp: resident_big_kernel):
//   word 0        the tag the workgroups post their records with (TreeParams::host_tag)
//   word 1        bits 0-1 operations (0-2) | bit 2 the stream ran something since the last command (re-read what it wrote) |
//                 bits 4-7 matrices to rebuild | bits 8-9 e_prefetch | bit 10 Update_Eigen_Lr, not an evaluation (edge_eval == 2) |
//                 bits 11-16 the large-grid evaluator's own (kBigDlk ... kBigGroupSum) | bits 17- host-computed matrices in the upload area
//   word 2        e_parent | e_child << 32
//   word 3        e_pm | last_dest << 32
//   words 4-5     the indices of the matrices to rebuild, or of the host-computed ones (never both kinds: up_ride), 32 bits each
//   words 6-9     the edge lengths of the matrices to rebuild (doubles)
//   words 10-33   per operation 12 words, a descriptor in two ({base, bytes | x << 32}): c1_data, c2_data, c1_scale, c2_scale,
//                 dst_data, dst_scale
//   word 34       20-state evaluator only: Instance::model_epoch (the caller sets it)
// `flags`: the route's own bits of word 1.  20-state commands never carry host-computed matrices or edge_eval == 2 (plan_route).
static void pack_command(unsigned long long *words, int n_words, const TreeParams &q, unsigned long long flags)
{
  memset(words, 0, sizeof(unsigned long long) * n_words);
  words[0] = q.host_tag;
  words[1] = (unsigned long long)q.n_real_ops | flags | ((unsigned long long)q.n_fresh << 4) | ((unsigned long long)q.e_prefetch << 8) |
             (q.edge_eval == 2 ? kBigEigen : 0ull) | ((unsigned long long)q.n_up << 17);
  words[2] = (unsigned long long)(unsigned)q.e_parent | ((unsigned long long)(unsigned)q.e_child << 32);
  words[3] = (unsigned long long)(unsigned)q.e_pm | ((unsigned long long)(unsigned)q.last_dest << 32);
  for (int k = 0; k < q.n_fresh; ++k)
  {
    words[4 + k / 2] |= (unsigned long long)(unsigned)q.fresh_idx[k] << (32 * (k & 1));
    memcpy(&words[6 + k], &q.fresh_len[k], 8);
  }
  for (int k = 0; k < q.n_up; ++k) words[4 + k / 2] |= (unsigned long long)(unsigned)q.up_idx[k] << (32 * (k & 1));
  auto put = [&](int k, const Desc &d) { words[k] = d.base; words[k + 1] = (unsigned long long)d.bytes | ((unsigned long long)d.x << 32); };
  for (int o = 0; o < q.n_real_ops; ++o)
  {
    put(10 + o * 12, q.arg_ir[o].c1_data); put(12 + o * 12, q.arg_ir[o].c2_data);
    put(14 + o * 12, q.arg_ir[o].c1_scale); put(16 + o * 12, q.arg_ir[o].c2_scale);
    put(18 + o * 12, q.arg_xr[o].dst_data); put(20 + o * 12, q.arg_xr[o].dst_scale);
  }
}

// The command goes to the resident workgroups.  What it was built from -- operations, matrix rebuilds, host-computed matrices --
// is kept until the answer is in: an evaluation nobody answers is launched the ordinary way (flush_and_wait)
static void send_command(Instance *I, Resident &R, const TreeParams &q, const unsigned long long *words, int n_words)
{
  I->sent.keep(I->pending, I->rebuilds, q);
  resident_send(I, R, words, n_words); // (every sector the workgroups wait for carries the command's number)
  I->rt_epoch = I->clean_epoch;
}

// What the workgroups of the two small resident evaluators are launched with: everything of the launch form's arguments that
// does not change per call (compared bytewise with Instance::rt_static)
static TreeParams resident_static_params(Instance *I)
{
  TreeParams sq = base_params(I);
  sq.host_blocks = I->h_blocks; sq.warn = I->h_warn; sq.fence_post = 1; sq.recs_in_args = 1; sq.edge_eval = 1;
  sq.br_len_mult = I->br_len_mult; sq.l_min = I->l_min; sq.l_max = I->l_max; sq.pmats_rw = I->d_pmats;
  if (I->soa) sq.dot_out = I->d_dot; // (nucleotides: they serve Update_Eigen_Lr too)
  if (I->want_site_outputs) { sq.site_lnl = I->d_site_lnl; sq.site_lk = I->d_site_lk; sq.site_cat = I->d_site_cat; }
  return sq;
}

// Do the workgroups of Instance::rt have to be launched for this geometry and these static arguments?  (A set launched with
// others is told to leave.)
static bool resident_stale(Instance *I, int grid, const TreeParams &sq)
{
  Resident  &R = I->rt;
  const bool differs = R.grid != grid || memcmp(&I->rt_static, &sq, sizeof sq) != 0;
  if (R.launched && !differs && !resident_gone(R)) return false;
  if (R.launched && differs) resident_stop(R);
  return true;
}

// The command of one of the two small evaluators, to the workgroups of Instance::rt
static void send_small(Instance *I, const FlushPlan &f, const TreeParams &q, int n_words)
{
  unsigned long long words[kResidentAaWords];
  static_assert(kResidentNtWords <= kResidentAaWords && kResidentAaWords == 35, "word 34: the 20-state evaluator's own");
  pack_command(words, n_words, q, I->clean_epoch != I->rt_epoch ? kBigChanged : 0ull); // (the stream ran something since the last command)
  if (I->perm) words[34] = I->model_epoch;
  send_command(I, I->rt, q, words, n_words);
  I->host_sum_n = f.host_sum_n; I->host_sum_ns = 1;
  retire_queue(I, f.fold_pm);
}

// ---- small 20-state alignments: the resident form of traverse_aa_kernel (phyhip_aa.hpp) -------------------------------------
static int send_resident_aa(Instance *I, const FlushPlan &f, const TreeParams &q)
{
  if (!(f.host_sum_n > 0 && q.recs_in_args && q.n_fresh <= 4 && q.n_up == 0))
    return fail(PHYHIP_ERROR_GENERAL, "20-state resident evaluator: an evaluation it cannot take (%d records, %d matrices)", f.host_sum_n, q.n_fresh);
  Resident        &R = I->rt;
  const TreeParams sq = resident_static_params(I);
  // geometry: as few workgroups as hold every wave-tile with at most kAaMaxCons2 consumers each, the tiles spread evenly
  const int ntl = I->grid_aa /* (aa_nw == 1: one tile per workgroup of the launched form) */, wgs = (ntl + kAaMaxCons2 - 1) / kAaMaxCons2,
            nwr = (ntl + wgs - 1) / wgs;
  if (resident_stale(I, wgs, sq))
  {
    AaResident  rs;
    hipStream_t st;
    if (const int rc = resident_prepare(I, R, wgs, kResidentAaWords, R.seq, rs.ctl, &st)) return rc;
    rs.evec = I->d_evec; rs.ivec = I->d_ivec; rs.eval = I->d_eval; rs.rates = I->d_catr; rs.pmats_rw = I->d_pmats; rs.afrag_rw = I->d_afrag;
    rs.stamps = nullptr; rs.stamp_wg = 0;
    if (getenv("PHYHIP_RESIDENT_STATS"))
    { // (where workgroup 0's time goes per command: printed when the instance goes)
      if (!I->d_big_stamps)
      {
        HIPCHK(hipMalloc((void **)&I->d_big_stamps, sizeof(unsigned long long) * 32));
        HIPCHK(hipMemsetAsync(I->d_big_stamps, 0, sizeof(unsigned long long) * 16, I->stream));
        HIPCHK(hipStreamSynchronize(I->stream));
      }
      rs.stamps = I->d_big_stamps;
      rs.stamp_wg = std::min(wgs - 1, std::max(0, atoi(getenv("PHYHIP_RESIDENT_STATS")) - 1));
    }
    if (launch_resident_aa(I->C, wgs, nwr, st, sq, (const double *)I->d_afrag, I->nmat_all, (const uint32_t *)I->d_tipmasks, rs))
      return fail(PHYHIP_ERROR_GENERAL, "20-state resident evaluator: no kernel for %d categories", I->C);
    HIPCHK(hipGetLastError());
    memcpy(&I->rt_static, &sq, sizeof sq);
    resident_launched(R, wgs);
  }
  send_small(I, f, q, kResidentAaWords);
  return 0;
}

// ---- small nucleotide alignments: the resident short-launch evaluator (resident_nt2_kernel) ------------------------
template <int C, int G> static void launch_resident_nt2(Instance *I, hipStream_t st, const TreeParams &sq, const ResidentCtl &r)
{
  hipLaunchKernelGGL((resident_nt2_kernel<C, G>), dim3(I->grid_nt2), dim3(64), 0, st, sq, r, (const double *)I->d_pmats,
                     (const uint8_t *)I->d_tipcodes, (const double *)I->d_evec, (const double *)I->d_ivec, (const double *)I->d_eval,
                     (const double *)I->d_catr);
}

// (taken = false, 0: the stream is not known to be idle, or the command's host-computed matrices found no upload area -- the
// ordinary launch takes the evaluation)
static int try_resident_nt2(Instance *I, const FlushPlan &f, const TreeParams &q, bool &taken)
{
  taken = false;
  if (!stream_clean_for_resident(I)) return 0;
  Resident        &R = I->rt;
  const TreeParams sq = resident_static_params(I);
  if (resident_stale(I, I->grid_nt2, sq))
  {
    ResidentCtl r;
    hipStream_t st;
    if (const int rc = resident_prepare(I, R, I->grid_nt2, kResidentNtWords, R.seq, r, &st)) return rc;
    switch (I->C * 8 + I->nt_groups)
    {
      case 1 * 8 + 1: launch_resident_nt2<1, 1>(I, st, sq, r); break;
      case 2 * 8 + 1: launch_resident_nt2<2, 1>(I, st, sq, r); break;
      case 2 * 8 + 2: launch_resident_nt2<2, 2>(I, st, sq, r); break;
      case 3 * 8 + 1: launch_resident_nt2<3, 1>(I, st, sq, r); break;
      case 4 * 8 + 1: launch_resident_nt2<4, 1>(I, st, sq, r); break;
      case 4 * 8 + 2: launch_resident_nt2<4, 2>(I, st, sq, r); break;
      default: return fail(PHYHIP_ERROR_GENERAL, "resident evaluator: no kernel for %d categories in %d groups", I->C, I->nt_groups);
    }
    HIPCHK(hipGetLastError());
    memcpy(&I->rt_static, &sq, sizeof sq);
    resident_launched(R, I->grid_nt2);
  }
  // (host-computed matrices and a record that turned out to live in host memory: the launch takes them in its arguments)
  if (q.n_up > 0 && !resident_push_uploads(R, q.n_up, q.up_val, 16 * I->C)) return 0;
  send_small(I, f, q, kResidentNtWords);
  taken = true;
  return 0;
}

// ---- profiling (phyhip_profile): HIP events around the launch, and what it must have moved ------------------------------------
static int prof_begin(Instance *I, hipEvent_t (&ev)[2])
{
  for (hipEvent_t &e : ev)
  { // (phyhip_profile(1) left a supply: creating an event costs about a microsecond of the step that is being timed)
    if (!I->prof_spare.empty()) { e = I->prof_spare.back(); I->prof_spare.pop_back(); }
    else HIPCHK(hipEventCreate(&e));
  }
  HIPCHK(hipEventRecord(ev[0], I->stream));
  return 0;
}

static int prof_end(Instance *I, hipEvent_t (&ev)[2], int n_queued)
{
  HIPCHK(hipEventRecord(ev[1], I->stream));
  I->prof_pairs.emplace_back(ev[0], ev[1]);
  I->prof_updates += (double)n_queued * (double)I->P;
  return 0;
}

// Minimum traffic of this launch if nothing but the kernel's own register forwarding saved a byte: every result is
// written once; a child is read unless it is a tip (1 byte per pattern) or forwarded in registers -- the reaches of the very
// step plan the operation records were written from.  (The pad of an odd list is not counted: it moves what its operation moved.)
static void account_traffic(Instance *I, const EdgeEval *ee, FlushPlan &f)
{
  const int       n_ops = f.n_ops;
  const bool      fat = f.fat;
  const double    rec = (double)I->C * I->S * 8.0 + 4.0;
  const double    bytes_of[5] = {1.0, 0.0, 0.0, 2.0 /* (an in-step child: its two tip bytes) */, rec}; // by Reach
  const StepPlan *plan = n_ops > 0 ? step_plan(I, f) : nullptr;
  double          rd = 0.0, wr = 0.0;
  for (int k = 0; k < n_ops; ++k)
  {
    if (plan[k].stored) wr += rec;
    for (int w = 0; w < 2; ++w) rd += bytes_of[(int)plan[k].reach[w]];
  }
  if (ee)
  { // root edge: both sides unless just produced, pattern weight in; per-pattern outputs out
    for (int c : {ee->parent, ee->child})
      rd += c < I->tips ? 1.0 : ((fat && n_ops > 0 && c == I->pending[n_ops - 1].dest) ? 0.0 : rec);
    rd += 8.0;
    wr += 4.0 + (I->want_site_outputs ? 16.0 + 8.0 * I->C : 0.0);
  }
  I->prof_rd_bytes += rd * (double)I->P;
  I->prof_wr_bytes += wr * (double)I->P;
}

// ---- large nucleotide alignments: the large-grid resident evaluator (resident_big_kernel) -------------------------------
// (launches of such an instance do not fence their stores before they post -- with megabytes of results in the L2s a
// write-back per wave costs more than the launch; whether the stream is idle again is found by querying it, big_clean)
// As a command to the resident workgroups (big_take), or the same kernel launched for this one evaluation (one_shot).
static int send_big(Instance *I, const EdgeEval *ee, const FlushPlan &f, const TreeParams &q)
{
  const int host_sum_n = f.host_sum_n;
  int       rc = 0;
  if (!(host_sum_n > 0 && q.recs_in_args && q.n_fresh <= 4 && (q.n_up == 0 || (f.big_take && q.n_fresh == 0))))
    return fail(PHYHIP_ERROR_GENERAL, "large-grid resident evaluator: an evaluation it cannot take (%d records, %d matrices)", host_sum_n, q.n_fresh);
  if (q.n_up > 0 && !resident_push_uploads(I->rb, q.n_up, q.up_val, 16 * I->C))
    return fail(PHYHIP_ERROR_GENERAL, "large-grid resident evaluator: no upload area for %d host-computed matrices", q.n_up);
  unsigned long long words[kBigWords];
  const bool changed = f.big_take && I->clean_epoch != I->rt_epoch; // the stream ran something since the last command
  const bool dsum = host_sum_n > I->big_device_sum;
  pack_command(words, kBigWords, q,
               (changed ? kBigChanged : 0ull) | (dsum ? kBigDeviceSum : 0ull) | (dsum && big_sum_by_group(I, host_sum_n) ? kBigGroupSum : 0ull));
  if (f.one_shot)
  { // launched, on the instance's stream: behind the resident workgroups' exit, if there are any (not when they were about
    // to be asked: there are none then, and the streak that launches them at its second call goes on)
    if (!f.big_try) big_release(I);
    I->touched_call = true;
    hipEvent_t pe[2] = {nullptr, nullptr};
    const bool timed = I->prof && !ee->eigen; // (Update_Eigen_Lr: the caller's own events are around this call)
    if (timed && (rc = prof_begin(I, pe))) return rc;
    if ((rc = big_one_shot(I, words, kBigWords))) return rc;
    if (timed) snprintf(I->prof_kernel, sizeof I->prof_kernel, "resident_big_kernel<%d, %d> (launched for one evaluation)", I->C, I->nt_groups);
    if (timed && (rc = prof_end(I, pe, f.n_queued))) return rc;
  }
  else
  {
    send_command(I, I->rb, q, words, kBigWords);
    I->fenced_eval = true; // (nothing went onto the stream: it is as idle as it was found)
  }
  I->host_sum_n = dsum ? 1 : host_sum_n; I->host_sum_ns = 1;
  retire_queue(I, f.fold_pm);
  // (launched: say when the stream is idle again, so that the resident workgroups can take the next one)
  if (f.one_shot && f.big_fit && (rc = stamp_stream(I))) return rc;
  return 0;
}

// ---- the traversal launch: which instantiation of which kernel ------------------------------------------------------------------
template <typename... A> static void named(Instance *I, const char *fmt, A... a)
{ // the kernel as a profiler names it (phyhip_profile_read_kernel)
  if (I->prof) snprintf(I->prof_kernel, sizeof I->prof_kernel, fmt, a...);
}

// every form of traverse_nt2_kernel / traverse_aa_kernel takes the same arguments
template <typename K> static void launch_nt2_form(K kernel, Instance *I, const FlushPlan &f, const TreeParams &q, unsigned long long *dbg = nullptr)
{
  hipLaunchKernelGGL(kernel, dim3(I->grid_nt2), dim3(64), 0, I->stream, q, f.d_irec, f.d_xrec, f.ro.pmats, f.ro.tip_codes, dbg);
}
template <typename K> static void launch_aa_form(K kernel, Instance *I, dim3 blk, const FlushPlan &f, const TreeParams &q, unsigned long long *dbg = nullptr)
{
  hipLaunchKernelGGL(kernel, dim3(I->grid_aa), blk, 0, I->stream, q, f.d_irec, f.d_xrec, (const double *)I->d_afrag, I->nmat_all,
                     (const uint32_t *)I->d_tipmasks, dbg, AaResident());
}

#ifdef PHYHIP_DIAG
// PHYHIP_ABLATE=8: the cycle stamps one wave left (the sixth launch's; costs a sync), printed to stderr
static int print_stamps(Instance *I, int n_steps, bool load_issue, int &printed, const std::vector<unsigned> *fl = nullptr)
{ // fl: the execute flags of a compact list (NtExec::fl): the step's kind and how its children reach it are printed beside its stamps
  if (printed++ != 5) return 0;
  unsigned long long h[64 * 8];
  HIPCHK(hipMemcpyAsync(h, I->d_dbg, sizeof h, hipMemcpyDeviceToHost, I->stream));
  HIPCHK(hipStreamSynchronize(I->stream));
  for (int k = 0; k < 64 && k < n_steps; ++k)
  {
    fprintf(stderr, "step %2d:", k);
    for (int i = 1; i < 7; ++i) fprintf(stderr, " %6lld", (long long)(h[k * 8 + i] - h[k * 8 + i - 1]));
    if (k + 1 < 64) fprintf(stderr, "  | next %6lld", (long long)(h[(k + 1) * 8] - h[k * 8 + 6]));
    if (load_issue) fprintf(stderr, "  | load issue %6lld of segment 4", (long long)(h[k * 8 + 7] - h[k * 8 + 3]));
    if (fl && k < (int)fl->size())
    {
      const unsigned x = (*fl)[(size_t)k];
      auto           how = [&](int s) { return (x & (kOpCh1 << s)) ? "in-step" : (x & (kOpTip1 << s)) ? "tip" : (x & (s ? kOpF21 : kOpF11)) ? "fwd1" : (x & (s ? kOpF22 : kOpF12)) ? "fwd2" : "loaded"; };
      fprintf(stderr, "  | kind %u: %s x %s%s", (x >> kRecKindShift) & 7u, how(0), how(1), (x & kRecStore) ? ", stored" : "");
    }
    fprintf(stderr, "\n");
  }
  return 0;
}

// timing-only ablations and stamped forms of the pipelined kernels (results invalid); kNotLaunched: none asked for
static int launch_nt2_diag(Instance *I, const FlushPlan &f, const TreeParams &q)
{
  if (!((I->ablate & 8) && I->C == 4 && I->nt_groups <= 2)) return kNotLaunched;
  if (!I->d_dbg) HIPCHK(hipMalloc((void **)&I->d_dbg, 64 * 8 * 8));
  // (a list with in-step children -- the mostly-unstored list a default traversal runs -- needs the instantiation that stages four matrices)
  if (I->nt_groups == 2 && f.has_inl) launch_nt2_form(traverse_nt2_kernel<4, 2, true, 0, 2, true>, I, f, q, I->d_dbg);
  else if (f.has_inl) return fail(PHYHIP_ERROR_NO_IMPLEMENTATION, "PHYHIP_ABLATE=8: the stamped form with in-step children is the two-lane one");
  else if (I->nt_groups == 2) launch_nt2_form(traverse_nt2_kernel<4, 2, true>, I, f, q, I->d_dbg);
  else launch_nt2_form(traverse_nt2_kernel<4, 1, true>, I, f, q, I->d_dbg);
  static int printed = 0;
  return print_stamps(I, q.n_ops, true, printed, &I->last_exec_fl);
}

static int launch_aa_diag(Instance *I, dim3 blk, const FlushPlan &f, const TreeParams &q)
{
  if (I->C == 4 && I->ablate >= 256)
  { // PHYHIP_ABLATE = 256 + bits: timing-only ablations of the 20-state kernel
#define AAABL(a_) case a_: launch_aa_form(traverse_aa_kernel<4, false, a_>, I, blk, f, q); return 0;
    switch (I->ablate - 256)
    {
      AAABL(1) AAABL(2) AAABL(4) AAABL(8) AAABL(9) AAABL(16) AAABL(18) AAABL(5) AAABL(13) AAABL(31) AAABL(27)
      default: break;
    }
#undef AAABL
  }
  if (!((I->ablate & 8) && I->ablate < 256 && I->C == 4)) return kNotLaunched;
  if (!I->d_dbg) HIPCHK(hipMalloc((void **)&I->d_dbg, 64 * 8 * 8));
  if (I->ablate & 128) launch_aa_form(traverse_aa_kernel<4, true, 31>, I, blk, f, q, I->d_dbg); // (stamps of the bare skeleton: every ablation on)
  else launch_aa_form(traverse_aa_kernel<4, true>, I, blk, f, q, I->d_dbg);
  static int printed = 0;
  return print_stamps(I, q.n_ops, false, printed);
}
#endif

// lane-per-pattern nucleotide kernel (phyhip_nt2.hpp), instantiated on the exact category count C and the lanes per pattern G
template <int C, int G> static void launch_nt2(Instance *I, const FlushPlan &f, const TreeParams &q)
{
  const bool list = !q.recs_in_args;
  if constexpr (C == 4 && G == 2)
    if (f.mixed)
    { // two wave shapes in one launch: full rounds of two-lane waves + four-lane waves for the rest
      named(I, "traverse_nt2_mixed_kernel<4, %s>", f.has_inl ? "true" : "false");
      auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(f.soa_grid), dim3(64), 0, I->stream, q, f.d_irec, f.d_xrec, f.ro.pmats, f.ro.tip_codes, I->mix_n2); };
      return f.has_inl ? go(traverse_nt2_mixed_kernel<4, true>) : go(traverse_nt2_mixed_kernel<4, false>);
    }
  if (list && I->prefetch_dist == 1)
  {
    named(I, "traverse_nt2_kernel<%d, %d, false, 0, 1>", C, G);
    return launch_nt2_form(traverse_nt2_kernel<C, G, false, 0, 1>, I, f, q);
  }
  if constexpr (G <= 2)
    if (list && f.has_inl)
    { // a list with in-step tip x tip children: the instantiation that stages four matrices per step
      named(I, "traverse_nt2_kernel<%d, %d, false, 0, 2, true>", C, G);
      return launch_nt2_form(traverse_nt2_kernel<C, G, false, 0, 2, true>, I, f, q);
    }
  // ARGS: 0 the list form; 1 / 2 operations in the kernel arguments; 3 none (the evaluation alone)
  const int args = list ? 0 : (q.n_real_ops == 1 ? 1 : (q.n_real_ops == 2 ? 2 : 3));
  named(I, "traverse_nt2_kernel<%d, %d, false, %d>", C, G, args);
  if (args == 0) launch_nt2_form(traverse_nt2_kernel<C, G, false, 0>, I, f, q);
  else if (args == 1) launch_nt2_form(traverse_nt2_kernel<C, G, false, 1>, I, f, q);
  else if (args == 2) launch_nt2_form(traverse_nt2_kernel<C, G, false, 2>, I, f, q);
  else launch_nt2_form(traverse_nt2_kernel<C, G, false, 3>, I, f, q);
}

static int launch_soa(Instance *I, const FlushPlan &f, const TreeParams &q)
{
#ifdef PHYHIP_DIAG
  if (const int rc = launch_nt2_diag(I, f, q); rc != kNotLaunched) return rc;
#endif
  switch (I->C * 8 + I->nt_groups)
  {
    case 1 * 8 + 1: launch_nt2<1, 1>(I, f, q); return 0;
    case 2 * 8 + 1: launch_nt2<2, 1>(I, f, q); return 0;
    case 2 * 8 + 2: launch_nt2<2, 2>(I, f, q); return 0;
    case 3 * 8 + 1: launch_nt2<3, 1>(I, f, q); return 0;
    case 4 * 8 + 1: launch_nt2<4, 1>(I, f, q); return 0;
    case 4 * 8 + 2: launch_nt2<4, 2>(I, f, q); return 0;
    case 4 * 8 + 4: launch_nt2<4, 4>(I, f, q); return 0;
    default: return kNotLaunched;
  }
}

// first-generation lane = (pattern, category) pipeline (phyhip_kernels.hpp): the production kernel for 5..8 categories
template <int CP> static void launch_nt(Instance *I, const FlushPlan &f, const TreeParams &q)
{
  named(I, "traverse_nt_kernel<%d, 0, %d>", CP, I->prefetch_dist == 1 ? 1 : 2);
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(I->grid_nt), dim3(I->block_nt), 0, I->stream, q, f.d_irec, f.d_xrec, f.ro.pmats, f.ro.tip_codes); };
  if (I->prefetch_dist == 1) return go(traverse_nt_kernel<CP, 0, 1>);
#ifdef PHYHIP_DIAG
  if constexpr (CP == 4)
    switch (I->ablate)
    { // PHYHIP_ABLATE: timing-only variants (results invalid)
#define ABLCASE(a) case a: return go(traverse_nt_kernel<CP, a>);
      ABLCASE(1) ABLCASE(2) ABLCASE(3) ABLCASE(6) ABLCASE(7)
#undef ABLCASE
      default: break;
    }
#endif
  go(traverse_nt_kernel<CP>);
}

// 20-state MFMA kernel (phyhip_aa.hpp): records in the arguments, a list with in-step children, or a plain list
template <int C> static void launch_aa(Instance *I, dim3 blk, const FlushPlan &f, TreeParams &q)
{
  const bool list = !q.recs_in_args, inl = list && f.has_inl;
  named(I, "traverse_aa_kernel<%d, false, 0, %s, %s, %d, %s>", C, list ? "false" : "true", inl ? "true" : "false", list ? I->aa_nt : 1,
        (list && I->aa_nt == 1 && I->aa_d2) ? "true" : "false");
  if constexpr (kDiag) // (measured variants of the list form, kept for A/B: profiles/r06_aa_kernel.md)
  {
    if (list && I->aa_nt == 1 && I->aa_d2)
    { // few waves per SIMD: loads two operations ahead
      if (inl) return launch_aa_form(traverse_aa_kernel<C, false, 0, false, true, 1, true>, I, blk, f, q);
      return launch_aa_form(traverse_aa_kernel<C, false, 0, false, false, 1, true>, I, blk, f, q);
    }
    if (list && I->aa_nt == 2)
    { // two wave-tiles per consumer wave
      const dim3 blk2(64 * ((I->aa_nw + 1) / 2 + 1));
      q.aa_tpw = I->aa_nw;
      if (inl) return launch_aa_form(traverse_aa_kernel<C, false, 0, false, true, 2>, I, blk2, f, q);
      return launch_aa_form(traverse_aa_kernel<C, false, 0, false, false, 2>, I, blk2, f, q);
    }
  }
  if (!list) return launch_aa_form(traverse_aa_kernel<C, false, 0, true>, I, blk, f, q);
  if (inl) return launch_aa_form(traverse_aa_kernel<C, false, 0, false, true>, I, blk, f, q);
  return launch_aa_form(traverse_aa_kernel<C>, I, blk, f, q);
}

static int launch_perm(Instance *I, const FlushPlan &f, TreeParams &q)
{
  const dim3 blk(64 * (I->aa_nw + 1));
#ifdef PHYHIP_DIAG
  if (const int rc = launch_aa_diag(I, blk, f, q); rc != kNotLaunched) return rc;
#endif
  switch (I->C)
  {
    case 1: launch_aa<1>(I, blk, f, q); return 0;
    case 2: launch_aa<2>(I, blk, f, q); return 0;
    case 3: launch_aa<3>(I, blk, f, q); return 0;
    case 4: launch_aa<4>(I, blk, f, q); return 0;
    default: return kNotLaunched;
  }
}

// The pipelined kernel of the instance's layout where one is instantiated for its shape, else the plain one.  (The guards
// bound what is instantiated per (S, CP) of dispatch_shape.)
static int launch_traversal(Instance *I, const FlushPlan &f, TreeParams &q)
{
  return dispatch_shape(I, [&](auto s, auto cp) {
    constexpr int S_ = decltype(s)::value, CP_ = decltype(cp)::value;
    if constexpr (S_ == 4 && CP_ <= 4)
      if (I->soa)
        if (const int rc = launch_soa(I, f, q); rc != kNotLaunched) return rc;
    if constexpr (S_ == 4 && CP_ <= 8 && (CP_ == 8 || kDiag))
      if (!I->generic_nt)
      {
        launch_nt<CP_>(I, f, q);
        return 0;
      }
    if constexpr (S_ == 20 && CP_ <= 4)
      if (I->perm)
        if (const int rc = launch_perm(I, f, q); rc != kNotLaunched) return rc;
    named(I, "traverse_kernel<%d, %d>", S_, CP_);
    hipLaunchKernelGGL((traverse_kernel<S_, CP_>), dim3(I->grid), dim3(256), 0, I->stream, q, f.ro.ops, f.ro.pmats, f.ro.tip_codes,
                       f.ro.code_masks);
    return 0;
  });
}

// Launch the queued operations (and optionally the fused edge evaluation) as one traversal kernel -- or hand them to resident
// workgroups that take such an evaluation without a launch.
static int flush_impl(Instance *I, const EdgeEval *ee)
{
  const unsigned long long hp0 = hp_now();
  FlushPlan f;
  f.n_queued = (int)I->pending.size();
  f.fat      = ((I->S == 4) && !I->generic_nt) || I->perm;
  // virtual buffers: what the queue reads of them is (re)computed in front of its reader; a long list of the two pipelined
  // kernels leaves results unstored as far as their register window reaches (rewrite_pending: two-deep forwarding)
  const bool unstoring = (I->soa || I->perm) && !I->generic_nt && !I->class_axis && !I->generic_loop && !(I->ablate & ~8) &&
                         !I->no_loads; // (PHYHIP_ABLATE=8 stamps the list a default traversal runs)
  rewrite_pending(I, ee, unstoring ? reg_window(I, f.fat, false) : RegWindow{0});
  I->unstored.keep_clear();
  const int n_ops = f.n_ops = (int)I->pending.size();
  int       rc = 0;
  if (n_ops > 0 || ee || !I->rebuilds.empty() || !I->uploads.empty()) I->stream_dirty = true;
  if (ee) I->fenced_eval = false;
  if ((rc = plan_route(I, ee, f))) return rc;
  if (!f.fold_pm && !f.up_ride && (!I->rebuilds.empty() || !I->uploads.empty()) && (rc = flush_pmats(I))) return rc;
  if (n_ops == 0 && !ee) return 0;
  if ((rc = upload_masks(I))) return rc;

  // ---- the kernel arguments: matrices, operation records, evaluation ----
  TreeParams q = base_params(I);
  f.ro      = base_ro(I, nullptr);
  f.has_inl = !I->pending_inl.empty();
  f.window  = reg_window(I, f.fat, f.big_cmd());
  fill_matrix_args(I, f, q);
  plan_aa_ring(I, ee, f, q);
  place_op_records(I, f);
  choose_list_kernel(I, f);
  if ((rc = build_op_records(I, f, q))) return rc;
  if (ee) setup_evaluation(I, ee, f, q);

  // ---- resident workgroups that take the evaluation without a launch, in the order they are tried ----
  const bool        rt_grid = resident_short_eligible(I);
  static const bool rtdbg = kDiag && getenv("PHYHIP_RESIDENT_DEBUG") != nullptr; // (diag build: why an evaluation was launched)
  if (rtdbg && ee)
    fprintf(stderr, "rt: grid_ok %d (res %d spin %d hs %d soa %d co %d cls %d g2 %d abl %d grp %d) hsn %d args %d fresh %d site %d prof %d skip %d dirty_prev %d touched %d\n",
            (int)rt_grid, (int)I->resident, (int)I->spin_wait, (int)I->host_sum, (int)I->soa, I->co != nullptr, (int)I->class_axis, I->grid_nt2,
            I->ablate, I->nt_groups, f.host_sum_n, q.recs_in_args, q.n_fresh, (int)I->want_site_outputs, (int)I->prof, (int)I->rt_skip,
            (int)I->dirty_prev, (int)I->touched_call);
  if ((rt_grid || resident_aa_eligible(I)) && f.host_sum_n > 0)
  { // every evaluation of such an instance completes its stores before it posts: the stream is clean once the scalar is back
    q.fence_post   = 1;
    I->fenced_eval = true;
  }
  if (f.aa_take) return send_resident_aa(I, f, q);
  if (rt_grid && f.host_sum_n > 0 && q.recs_in_args && q.n_fresh <= 4 && (q.n_up == 0 || up_resident(I, f, I->rt)) && !I->prof && !I->rt_skip)
  {
    bool taken = false;
    if ((rc = try_resident_nt2(I, f, q, taken)) || taken) return rc;
  }
  if (f.big_cmd()) return send_big(I, ee, f, q);

  // ---- the ordinary launch ----
  if (!f.big_try) big_release(I); // (what follows needs the wave slots the large-grid resident workgroups hold, if there are any)
  I->touched_call = true; // (everything below goes onto the stream)
  hipEvent_t pe[2] = {nullptr, nullptr};
  if (I->prof && (rc = prof_begin(I, pe))) return rc;
  const unsigned long long hp1 = hp_now();
  if ((rc = launch_traversal(I, f, q))) return rc;
  if (I->prof)
  {
    if ((rc = prof_end(I, pe, f.n_queued))) return rc;
    account_traffic(I, ee, f);
  }
  if (kDiag) { const unsigned long long hp2 = hp_now(); g_hp.prep += hp1 - hp0; g_hp.launch += hp2 - hp1; ++g_hp.n_launch; }
  HIPCHK(hipGetLastError());
  I->host_sum_n = f.host_sum_n; I->host_sum_ns = 1;
  if (ee && !ee->eigen && !f.fused_sum && !f.host_sum_n && !I->class_axis) // (class axis: the combination kernel follows, no sum here)
  {
    double *out = ee->dev_out ? ee->dev_out : I->d_result;
    const int nsum = I->soa ? f.soa_grid : (I->perm ? I->grid_aa : (f.fat ? I->grid_nt : I->grid));
    hipLaunchKernelGGL(final_reduce_kernel, dim3(1), dim3(256), 0, I->stream, (const double *)I->d_block, nsum, 1,
                       nsum, out, ee->to_host ? I->h_result : (double *)nullptr, I->d_warn, I->h_warn,
                       ee->to_host ? ++I->seq : 0ull, ee->warn_out);
    HIPCHK(hipGetLastError());
  }
  retire_queue(I, f.fold_pm);
  // an evaluation the large-grid resident workgroups would have taken, had the stream been known to be idle: say when it is
  if (f.big_fit && f.host_sum_n > 0 && (rc = stamp_stream(I))) return rc;
  return 0;
}

int flush(Instance *I, const EdgeEval *ee)
{
  const int rc = flush_impl(I, ee);
  // a failed launch leaves no half-queued state behind: the operations are dropped (the caller gets the error and
  // PhyML's glue exits on it), queued matrix rebuilds stay queued, no device slot claims a list it never received
  if (rc) retire_queue(I, false);
  return rc;
}

int flush_sync(Instance *I)
{
  int rc = flush(I, nullptr);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(I->stream));
  return 0;
}

int check_partial_index(const Instance *I, int idx, bool allow_tip)
{
  if (idx < 0 || idx >= I->nbuf || (!allow_tip && idx < I->tips))
    return fail(PHYHIP_ERROR_OUT_OF_RANGE, "partials buffer index %d out of range [%d,%d)", idx, allow_tip ? 0 : I->tips, I->nbuf);
  return 0;
}

// Wait until the final reduction has published evaluation `seq` in host-mapped memory.  Spinning on the
// sequence word avoids the stream-synchronise wake-up latency; after 2 ms of spinning (elapsed time, checked every
// 256 polls) fall back to it: evaluations of very large alignments take milliseconds and must not burn a core.
// The host's side of the final sum on large grids: poll the {sum, tag} records the workgroups posted (they arrive roughly in
// launch order), then add them exactly as final_reduce_kernel does -- 256 strided accumulators, then a binary tree -- so
// that the value does not depend on which path produced it.
int wait_host_sum(Instance *I)
{
  const int                n   = I->host_sum_n * I->host_sum_ns, per = I->host_sum_n;
  const unsigned long long tag = I->seq;
  volatile HostBlock      *hb  = I->h_blocks;
  struct timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  bool   synced = false;
  // final_reduce_kernel's order -- 256 strided accumulators per sum, then a binary tree -- with the records taken as they
  // arrive, front to back: accumulator t receives records t, t + 256, ... in that order either way, and one sequential pass
  // over the records costs a fraction of 256 strided ones (thousands of records per evaluation on large grids)
  double acc[2][256];
  for (int k = 0; k < I->host_sum_ns; ++k)
    for (int t = 0; t < 256; ++t) acc[k][t] = 0.0;
  for (int i = 0, k = 0, j = 0; i < n; ++i)
  {
    long it = 0;
    while (hb[i].tag != tag)
    {
      __builtin_ia32_pause();
      if ((++it & 255) == 0 && !synced)
      {
        struct timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const long waited = (t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec);
        if (I->r_inflight)
        { // no answer from the resident workgroups (they may have left just before the command arrived): the caller
          // retires them and launches the evaluation the ordinary way
          if (waited > 30000L && resident_gone(*I->r_inflight)) return kResidentSilent; // they left as the command arrived
          // (a healthy command of the large-grid evaluator takes ~8 ns per tile and operation -- 25 us at 3 126 tiles -- so the
          // give-up time grows with the grid: 100 us + 80 ns per tile)
          const long patience = 100000L + (I->r_inflight == &I->rb ? 80L * (long)I->grid_nt2 : 0L);
          if (waited > patience && ns_since(I->r_inflight->t_launch) > 20e6) return kResidentSilent; // (a first launch loads code: ms)
          continue;
        }
        if (waited > 2000000L || !I->spin_wait)
        {
          HIPCHK(hipStreamSynchronize(I->stream));
          synced = true;
          it = 0;
        }
      }
      else if (synced && it > 100000000L)
        return fail(PHYHIP_ERROR_GENERAL, "evaluation %llu finished without posting block sum %d", tag, i);
    }
    acc[k][j & 255] += hb[i].sum; // (the record is ONE 16-byte store of the device: the sum is there when the tag is)
    if (++j == per) { j = 0; ++k; }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  for (int k = 0; k < I->host_sum_ns; ++k)
  {
    for (int off = 128; off > 0; off >>= 1)
      for (int t = 0; t < off; ++t) acc[k][t] += acc[k][t + off];
    I->h_result[k] = acc[k][0];
  }
  I->host_sum_n    = 0;
  if (I->r_inflight) I->r_inflight->ns_wait += ns_since(I->r_inflight->t_cmd);
  I->r_inflight    = nullptr;
  I->warn_current  = true;
  *reinterpret_cast<volatile unsigned long long *>(I->h_result + 2) = tag;
  return 0;
}

static int wait_result_impl(Instance *I)
{
  if (I->host_sum_n > 0) return wait_host_sum(I);
  if (I->spin_wait)
  {
    volatile unsigned long long *flag = reinterpret_cast<volatile unsigned long long *>(I->h_result + 2);
    struct timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long it = 0;; ++it)
    {
      if (*flag == I->seq)
      {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        I->warn_current = true;
        return 0;
      }
      __builtin_ia32_pause();
      if ((it & 255) == 255)
      {
        struct timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 2000000L) break;
      }
    }
  }
  HIPCHK(hipStreamSynchronize(I->stream));
  if (*reinterpret_cast<volatile unsigned long long *>(I->h_result + 2) != I->seq)
  { // the stream drained without the hand-over (a faulted launch): do not return a stale scalar, re-arm the ticket counter
    (void)hipMemsetAsync(I->d_tickets, 0, sizeof(unsigned) * (1 + kTicketGroups), I->stream);
    return fail(PHYHIP_ERROR_GENERAL, "evaluation %llu finished without handing its result over", I->seq);
  }
  I->warn_current = true;
  return 0;
}

int wait_result(Instance *I)
{
  const unsigned long long t0 = hp_now();
  const int rc = wait_result_impl(I);
  if (kDiag) { const unsigned long long t1 = hp_now(); g_hp.wait += t1 - t0; ++g_hp.n_wait; if (!g_hp.t_first) g_hp.t_first = t0; g_hp.t_last = t1; }
  return rc;
}

int collect_profile(Instance *I)
{
  for (auto &pr : I->prof_pairs)
  {
    HIPCHK(hipEventSynchronize(pr.second));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
    I->prof_ms += ms;
    I->prof_n += 1;
    for (hipEvent_t e : {pr.first, pr.second})
      if (I->prof_spare.size() < 1024) I->prof_spare.push_back(e);
      else (void)hipEventDestroy(e);
  }
  I->prof_pairs.clear();
  for (auto &pr : I->prof_aux)
  {
    HIPCHK(hipEventSynchronize(pr.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pr.a, pr.b));
    I->prof_aux_ms[pr.kind] += ms;
    I->prof_aux_n[pr.kind] += 1;
    (void)hipEventDestroy(pr.a);
    (void)hipEventDestroy(pr.b);
  }
  I->prof_aux.clear();
  return 0;
}

// The command nobody answered, back into the queue: its operations (and the matrices they read), the rebuilds it folded unless
// the matrix has been queued since, then its host-computed matrices as phyhip_set_transition_matrix queued them
static int requeue_sent(Instance *I)
{
  SentCommand &c = I->sent;
  I->pending = c.ops;
  for (const DevOp &o : I->pending) mark_matrix_readers(I, o.pm1, o.pm2);
  for (size_t k = 0; k < c.pm_idx.size(); ++k) I->rebuilds.put_if_absent(c.pm_idx[k], c.pm_len[k]);
  for (int k = 0; k < c.n_up; ++k)
  {
    const size_t bytes = (size_t)I->C * I->S * I->S * sizeof(double);
    void        *st = nullptr;
    if (int rc = I->ring.alloc(bytes, I->stream, &st)) return rc;
    memcpy(st, c.up_val[k], bytes);
    I->uploads.put_if_absent(c.up_idx[k], (const double *)st); // (absent: the command took every queued upload)
  }
  c.n_up = 0;
  return 0;
}

// An evaluation the host waits for (edge sum, or the empty records of a small alignment's Update_Eigen_Lr): queue, launch or
// hand to the resident short-launch evaluator, wait.  An evaluation the resident workgroups do not answer is launched.
int flush_and_wait(Instance *I, EdgeEval &ee, bool flushed)
{
  int rc = flushed ? 0 : flush(I, &ee);
  if (rc) return rc;
  Resident  *const by = I->r_inflight;
  const bool by_resident = by != nullptr;
  rc = wait_result(I);
  if (rc == kResidentSilent)
  { // the resident workgroups had left: retire them for good (no late record can arrive after this), put the evaluation
    // back in the queue and launch it
    ++by->n_silent;
    resident_stop(*by);
    if (by == &I->rb) big_release(I);
    I->r_inflight = nullptr; I->host_sum_n = 0;
    if ((rc = requeue_sent(I))) return rc;
    I->rt_skip = true;
    rc = flush(I, &ee);
    I->rt_skip = false;
    if (rc) return rc;
    rc = wait_result(I);
  }
  if (rc) return rc;
  if (I->fenced_eval)
  { // every store of this evaluation -- and so everything queued before it -- is in memory
    I->fenced_eval = false; I->stream_dirty = false; I->clean_after = 0;
    // (a kernel ran, or the small evaluators' dot_prod was rewritten by another set of workgroups: they re-read.  Not the
    // large-grid evaluator's: the wave that evaluates a tile's dLk is the one that wrote its products, phyhip_big.hpp)
    if (!by_resident || (ee.eigen && by != &I->rb)) ++I->clean_epoch;
  }
  return 0;
}

} // namespace phyhip_host

