// tests/records_model.hip -- test infrastructure (CPU only, no device is touched): the operation records the kernels read, decoded
// back and held against the step plan they were written from (phyml_amd/csrc/phyhip_step_plan.hpp).  The whole text of
// phyml_amd/csrc/phyhip_queue.hip is compiled into this program (QUEUE_UNIT names it), so that its encoders -- fill_records with
// child_descs, fill_compact_records -- are called as flush_impl calls them, on an Instance built by hand whose device pointers are
// made-up addresses: the encoders compute with them and never look behind them.  For seeded random lists (post-orders with in-step
// children, non-storing re-issues and results that are not stored, odd and even lengths) it decodes IssueRec / ExecRec and
// NtIssue / NtExec back to a reach per child and a store bit and requires
//   * both encodings say what the plan says, record for record, and load exactly the children the plan calls Loaded, from their
//     own buffers;
//   * the kOp* flag words of the two encodings are equal;
//   * a compact record's step kind is kind_of of the plan over the rows that are one-hot (and the kind its documentation names),
//     or 0 throughout where the list's kernel carries no step bodies.
// Shapes: 4 states, 4 categories in 1, 2 and 4 lanes per pattern (the two-lane shape also with two wave shapes: the mixed kernel),
// and 20 states, 4 categories (descriptors only) -- each with and without in-step children where the kernels have them; and, for the
// shallower windows, the two-lane shape with loads one operation ahead and one or two operations as a large-grid command.
// Built and run through tests/test_records_plan.py:  records_model <file for the record bytes, or -> [lists per shape]
#include QUEUE_UNIT

#include <random>

using namespace phyhip_host;

// The unit's launch stubs refer to the device code of its kernels, which a host-only compilation does not have: the link points
// that symbol here (tests/test_records_plan.py) -- a code object bundle with no entries.  Nothing in this program launches.
extern "C" { alignas(4096) extern const unsigned char records_model_no_kernels[32] = "__CLANG_OFFLOAD_BUNDLE__"; }

[[noreturn]] static void die(const char *what, int shape, long list, int rec, int s)
{
  fprintf(stderr, "RECORDS_MODEL FAIL: %s (shape %d, list %ld, record %d, child %d)\n", what, shape, list, rec, s);
  exit(1);
}

struct Shape
{
  int  S, G;
  bool in_step, mixed;
  int  dist = 2;    // loads that many operations ahead: the depth of the register window
  bool big = false; // one or two operations as a command for the large-grid evaluator: no forwarding at all
};
static const Shape kShapes[] = {{4, 1, false, false}, {4, 1, true, false}, {4, 2, false, false}, {4, 2, true, false}, {4, 2, false, true},
                                {4, 2, true, true},   {4, 4, false, false}, {20, 1, false, false}, {20, 1, true, false},
                                {4, 2, false, false, 1}, {4, 1, false, false, 2, true}};

// made-up arena addresses (never dereferenced)
static const uintptr_t kPartials = 0x100000000000ull, kScales = 0x200000000000ull, kTipcodes = 0x300000000000ull, kTipmasks = 0x400000000000ull;

static Instance *make_instance(const Shape &sh, int tips)
{
  Instance *I = new Instance();
  I->tips = tips; I->nbuf = 3 * tips; I->S = sh.S; I->C = 4; I->NE = 1;
  I->soa = sh.S == 4; I->perm = sh.S == 20; I->nt_groups = sh.G; I->prefetch_dist = sh.dist;
  I->P = 100; I->Ppad = I->perm ? 112 : 128;
  I->d_partials = reinterpret_cast<decltype(I->d_partials)>(kPartials); I->d_scales = reinterpret_cast<decltype(I->d_scales)>(kScales);
  I->d_tipcodes = reinterpret_cast<decltype(I->d_tipcodes)>(kTipcodes); I->d_tipmasks = reinterpret_cast<decltype(I->d_tipmasks)>(kTipmasks);
  I->grid_nt2 = (int)(I->Ppad / (64 / I->nt_groups));
  if (sh.mixed) { I->mix_n2 = 2; I->mix_n4 = 3; }
  if (I->soa)
  { // the host's mirror of the tip rows: every third row carries an ambiguous code (tip_row_bits: not one-hot)
    I->h_tiprows.assign((size_t)tips * I->P, 1);
    I->tip_namb.assign((size_t)tips, 0); I->tip_n15.assign((size_t)tips, 0);
    for (int t = 0; t < tips; t += 3) I->tip_namb[(size_t)t] = 1;
  }
  return I;
}

// A post-order as a traversal emits one, rewritten the way rewrite_pending leaves lists: a tip child may have become a virtual
// buffer (2 tips .. 3 tips - 1) computed in-step (one per operation) or re-issued in front, not storing; some results are unstored
static void random_list(std::mt19937 &rng, Instance *I, bool in_step, bool two_at_most)
{
  auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
  const int tips = I->tips, n_ops = two_at_most ? 1 + rnd(2) : 1 + rnd(tips - 1), nmat = 2 * tips;
  std::vector<DevOp>     &L = I->pending;
  std::vector<InlineDef> &D = I->pending_inl;
  std::vector<int>        open;
  L.clear(); D.clear();
  const InlineDef none{-1, -1, -1, -1};
  int             next_virt = 0;
  bool            any = false;
  for (int k = 0; k < n_ops; ++k)
  {
    auto take = [&](bool newest) {
      if (open.empty() || rnd(3) == 0) return rnd(tips);
      const size_t at = (newest || rnd(3)) ? open.size() - 1 : (size_t)rnd((int)open.size());
      const int    c = open[at];
      open.erase(open.begin() + (long)at);
      return c;
    };
    DevOp     o{tips + k, take(true), take(false), rnd(nmat), rnd(nmat), rnd(4) == 0 ? kOpNoStore : 0};
    InlineDef d = none;
    for (int s = 0; s < 2; ++s)
    {
      int &c = s ? o.c2 : o.c1;
      if (c >= tips || rnd(3) || next_virt >= tips || two_at_most) continue;
      const int v = 2 * tips + next_virt++;
      if (in_step && d.a < 0 && rnd(2)) { c = v; o.pad |= s ? kOpInl2 : kOpInl1; d = InlineDef{rnd(tips), rnd(tips), rnd(nmat), rnd(nmat)}; any = true; }
      else { c = v; L.push_back(DevOp{v, rnd(tips), rnd(tips), rnd(nmat), rnd(nmat), kOpNoStore}); D.push_back(none); }
    }
    L.push_back(o); D.push_back(d);
    open.push_back(o.dest);
  }
  if (!any) D.clear(); // (as rewrite_pending leaves it: empty unless some operation has an in-step child)
}

// the kind a step's documentation names (NtExec::fl, phyhip_kernels.hpp), said independently of kind_of's table
static unsigned documented_kind(Reach a, Reach b)
{
  const Reach T = Reach::Tip, F = Reach::Prev1, N = Reach::InStep;
  return (a == T && b == F) ? 1u : (a == F && b == T) ? 2u : (a == N && b == F) ? 3u : (a == F && b == N) ? 4u : (a == N && b == T) ? 5u : (a == T && b == N) ? 6u : 0u;
}

static Reach reach_of_flags(unsigned fl, int s)
{
  if (fl & (kOpCh1 << s)) return Reach::InStep;
  if (fl & (kOpTip1 << s)) return Reach::Tip;
  if (fl & (s ? kOpF21 : kOpF11)) return Reach::Prev1;
  if (fl & (s ? kOpF22 : kOpF12)) return Reach::Prev2;
  return Reach::Loaded;
}

int main(int argc, char **argv)
{
  FILE     *dump = (argc > 1 && strcmp(argv[1], "-") != 0) ? fopen(argv[1], "wb") : nullptr;
  const int lists_per_shape = argc > 2 ? atoi(argv[2]) : 300;
  long      n_lists = 0, n_desc = 0, n_compact = 0, n_kinds[kNtStepKinds] = {0}, n_reach[5] = {0}, n_unstored = 0, n_pads = 0;
  const unsigned kOpBits = kOpTip1 | kOpTip2 | kOpF11 | kOpF12 | kOpF21 | kOpF22 | kOpCh1 | kOpCh2;
  for (int shape = 0; shape < (int)(sizeof kShapes / sizeof kShapes[0]); ++shape)
  {
    const Shape &sh = kShapes[shape];
    std::mt19937 rng(1000u + (unsigned)shape);
    for (int rep = 0; rep < lists_per_shape; ++rep, ++n_lists)
    {
      Instance *I = make_instance(sh, 3 + (rep % 38));
      random_list(rng, I, sh.in_step, sh.big);
      // ---- as flush_impl, from the rewritten queue to the records ----
      FlushPlan  f;
      TreeParams q;
      memset(&q, 0, sizeof q);
      f.n_ops = (int)I->pending.size();
      f.fat = true;
      f.big_take = sh.big;
      f.has_inl = !I->pending_inl.empty();
      f.window = reg_window(I, f.fat, f.big_cmd());
      plan_aa_ring(I, nullptr, f, q);
      f.compact = compact_list_form(I) && !f.big_cmd();
      choose_list_kernel(I, f);
      const int       n_rec = padded_records(f.n_ops);
      const StepPlan *plan = step_plan(I, f);
      std::vector<IssueRec> ir((size_t)n_rec);
      std::vector<ExecRec>  xr((size_t)n_rec);
      std::vector<NtIssue>  cir((size_t)n_rec);
      std::vector<NtExec>   cxr((size_t)n_rec);
      memset(ir.data(), 0, sizeof(IssueRec) * n_rec); memset(xr.data(), 0, sizeof(ExecRec) * n_rec);
      fill_records(I, f, plan, ir.data(), xr.data(), n_rec);
      if (f.compact && fill_compact_records(I, f, plan, cir.data(), cxr.data(), n_rec)) die("fill_compact_records refused the list", shape, rep, -1, -1);
      if (f.mixed != sh.mixed || (sh.S == 20 && f.compact)) die("the shape is not the one asked for", shape, rep, -1, -1);
      // ---- decoded, against the plan ----
      n_pads += n_rec - f.n_ops;
      for (int k = 0; k < n_rec; ++k)
      {
        const StepPlan &p = plan[k];
        const DevOp    &o = I->pending[(size_t)p.op];
        const unsigned  dfl = xr[(size_t)k].dst_data.x;
        ++n_desc;
        if ((xr[(size_t)k].dst_data.bytes != 0) != p.stored || (xr[(size_t)k].dst_scale.bytes != 0) != p.stored) die("descriptor records: the store", shape, rep, k, -1);
        n_unstored += !p.stored;
        if (xr[(size_t)k].dst_data.base != kPartials + (size_t)(o.dest - I->tips) * buf_elems(I) * sizeof(double)) die("descriptor records: the destination", shape, rep, k, -1);
        bool onehot[2] = {false, false};
        for (int s = 0; s < 2; ++s)
        {
          const int   c = s ? o.c2 : o.c1;
          const Desc &data = s ? ir[(size_t)k].c2_data : ir[(size_t)k].c1_data, &scale = s ? ir[(size_t)k].c2_scale : ir[(size_t)k].c1_scale;
          ++n_reach[(int)p.reach[s]];
          if ((p.reach[s] == Reach::Prev1 && sh.dist * !sh.big < 1) || (p.reach[s] == Reach::Prev2 && sh.dist * !sh.big < 2)) die("a child is forwarded beyond the window", shape, rep, k, s);
          if (reach_of_flags(dfl, s) != p.reach[s]) die("descriptor records: how a child reaches its step", shape, rep, k, s);
          const bool loaded = p.reach[s] == Reach::Loaded;
          if ((data.bytes != 0) != loaded || (loaded && data.base != kPartials + (size_t)(c - I->tips) * buf_elems(I) * sizeof(double)))
            die("descriptor records: a child's data load", shape, rep, k, s);
          if (loaded && (scale.bytes == 0 || scale.base != kScales + (size_t)(c - I->tips) * scale_elems(I) * 4)) die("descriptor records: a loaded child's scale vector", shape, rep, k, s);
          if ((p.reach[s] == Reach::Prev1 || p.reach[s] == Reach::Prev2) && scale.bytes != 0) die("descriptor records: a forwarded child loads", shape, rep, k, s);
          if (I->soa)
          {
            const InlineDef *d = p.reach[s] == Reach::InStep ? &I->pending_inl[(size_t)p.op] : nullptr;
            onehot[s] = d ? (tip_row_bits(I, d->a) & 1) && (tip_row_bits(I, d->b) & 1) : p.reach[s] == Reach::Tip && (tip_row_bits(I, c) & 1);
          }
        }
        if (!f.compact) continue;
        ++n_compact;
        const unsigned cfl = cxr[(size_t)k].fl, ifl = cir[(size_t)k].fl;
        if ((cfl & kOpBits) != (dfl & kOpBits)) die("the kOp flag words of the two encodings differ", shape, rep, k, -1);
        if (((cfl & kRecStore) != 0) != p.stored) die("compact records: the store", shape, rep, k, -1);
        if (cxr[(size_t)k].dst_data != (unsigned)((size_t)(o.dest - I->tips) * buf_elems(I) * sizeof(double) / 16)) die("compact records: the destination", shape, rep, k, -1);
        for (int s = 0; s < 2; ++s)
        {
          const int   c = s ? o.c2 : o.c1;
          const Reach got = (ifl & (kRecIn1 << s)) ? Reach::InStep : (ifl & (kRecT1 << s)) ? Reach::Tip : (ifl & (kRecL1 << s)) ? Reach::Loaded
                            : (cfl & (s ? kOpF21 : kOpF11)) ? Reach::Prev1 : (cfl & (s ? kOpF22 : kOpF12)) ? Reach::Prev2 : Reach::Loaded;
          if (got != p.reach[s] || reach_of_flags(cfl, s) != p.reach[s]) die("compact records: how a child reaches its step", shape, rep, k, s);
          const bool loaded = p.reach[s] == Reach::Loaded;
          if (((ifl & (kRecL1 << s)) != 0) != loaded || (loaded && cir[(size_t)k].data[s] != (unsigned)((size_t)(c - I->tips) * buf_elems(I) * sizeof(double) / 16)))
            die("compact records: a child's data load", shape, rep, k, s);
          if (((ifl & (kRecA1 << s)) != 0) != (loaded || p.reach[s] == Reach::Tip || p.reach[s] == Reach::InStep)) die("compact records: a child's auxiliary load", shape, rep, k, s);
        }
        const unsigned kind = (cfl >> kRecKindShift) & 7u, want = f.bodied ? kind_of(p, onehot) : 0u;
        if (kind != want) die("compact records: the step's kind is not kind_of of the plan over one-hot rows", shape, rep, k, -1);
        if (f.bodied && kind != ((onehot[0] || p.reach[0] == Reach::Prev1) && (onehot[1] || p.reach[1] == Reach::Prev1) ? documented_kind(p.reach[0], p.reach[1]) : 0u))
          die("compact records: the step's kind is not the one its documentation names", shape, rep, k, -1);
        ++n_kinds[kind];
      }
      if (dump)
      {
        fwrite(ir.data(), sizeof(IssueRec), (size_t)n_rec, dump); fwrite(xr.data(), sizeof(ExecRec), (size_t)n_rec, dump);
        if (f.compact) { fwrite(cir.data(), sizeof(NtIssue), (size_t)n_rec, dump); fwrite(cxr.data(), sizeof(NtExec), (size_t)n_rec, dump); }
        fwrite(I->rec_stats, sizeof I->rec_stats, 1, dump); fwrite(I->step_kinds, sizeof I->step_kinds, 1, dump);
      }
      delete I;
    }
  }
  if (dump) fclose(dump);
  for (int x = 0; x < 5; ++x)
    if (!n_reach[x]) die("a reach never occurred", -1, n_lists, -1, x);
  for (int k = 0; k <= 6; ++k)
    if (!n_kinds[k]) die("a step kind never occurred", -1, n_lists, -1, k);
  if (!n_unstored || !n_pads) die("no unstored result, or no padded list", -1, n_lists, -1, -1);
  printf("RECORDS_MODEL OK: lists %ld, descriptor_records %ld, compact_records %ld, pads %ld, unstored %ld, kinds %ld %ld %ld %ld %ld %ld %ld\n", n_lists, n_desc,
         n_compact, n_pads, n_unstored, n_kinds[0], n_kinds[1], n_kinds[2], n_kinds[3], n_kinds[4], n_kinds[5], n_kinds[6]);
  return 0;
}
