// tests/unstored_model.hip -- test infrastructure (CPU only, no device is touched): the symbolic model of the unstored-buffer
// bookkeeping of libphyhip.so (phyml_amd/csrc/phyhip_unstored.hip: rewrite_pending, devirtualise*, settle_deferred, defer_forwarded;
// the table: Unstored, phyhip_host.hpp).  It links the BUILT library, builds an Instance by hand -- the table sized as
// phyhip_create_instance sizes it --, feeds it random queues, readers and writers, and after every "launch" interprets the rewritten
// queue with the kernels' forwarding rules (last two results in registers, in-step children, non-storing operations) on symbolic
// values, in lockstep with the plain semantics (every operation stored, in queue order):
//   * a stale buffer must never be read from memory; the evaluation edge sees the plain semantics' values;
//   * what a launch leaves in memory -- or unstored, through its definition -- must be what the plain semantics hold for that buffer;
//   * the step plan of the rewritten queue (phyhip_step_plan.hpp: what the record encoders read) must say of every child what this
//     interpretation says of it, register for register, and must load nothing that is stale.
// The first argument is the highest class of unstored buffer switched on; the checks and events that depend on it:
//   1  virtual.  Every written buffer is stored or virtual.
//   2  + deferred (Unstored::defer_stores).  A deferred definition's inputs are in memory and are the plain values they had when the
//      definition was made; its value over them is the buffer's plain value; the counters match the classes.  Events: replayed
//      post-orders (they rewrite inputs and buffers in the order a repeated Lk(NULL) does), short lists that write an input of a
//      deferred buffer.
//   3  + chained (Unstored::chain_min_ops).  Instead of class 2's input checks: the definition of every unstored buffer, evaluated
//      over its inputs' definitions recursively, is the buffer's plain value; every input of a deferred or chained definition is a
//      tip, stored, or unstored under an older sequence number.  Events: the replayed post-orders give every edge its own matrix
//      (the lists that chain); short lists that write a buffer in the middle of a chain; a reader of a chain's last buffer before
//      any reader of its first -- across launches and inside one queue, in both orders --; readers that rewrite the queue once
//      without launching it before the launch rewrites it again (phyhip_update_eigen_lr).
// Matrices and tip rows change through the store-first route (devirtualise_matrix / devirtualise_tip + a launch); the snapshot
// route of the matrix setters needs a device and is covered by tests/test_gpu_virtual.py.
// Built and run through tests/unstored_model.py:  unstored_model <class 1|2|3> <seed> <events> <tips> <soa 0|1> [in-step children 1|0]
#include "../phyml_amd/csrc/phyhip_host.hpp"

#include <algorithm>
#include <cstdint>
#include <random>

using namespace phyhip_host;
using U = Unstored;

static uint64_t H(uint64_t a, uint64_t b, uint64_t c, uint64_t d)
{
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (uint64_t v : {a, b, c, d})
  {
    x ^= v + 0x9e3779b97f4a7c15ull + (x << 6) + (x >> 2);
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 31;
  }
  return x;
}

struct Model
{
  Instance *I;
  int       cls;                        // the highest class switched on
  std::vector<uint64_t> tipv, matv;     // versions of the tip rows / matrices
  std::vector<uint64_t> ref, dev;       // plain semantics / device memory per buffer
  std::vector<char>     written;        // the buffer has been the destination of a queued operation
  std::vector<DevOp>    queued;         // what the caller queued since the last launch (plain semantics are applied at launch)
  std::vector<char>     was_def;        // below class 3: the buffer was deferred after the previous launch
  std::vector<DevOp>    seen_def;       // ... with this definition
  std::vector<uint64_t> in1, in2;       // ... whose inputs had these plain values when it was made
  long                  n_launch = 0, n_instep = 0, n_nostore = 0, n_pad = 0;
  mutable long          max_chain = 0;

  const Unstored &u() const { return I->unstored; }
  bool is(int b, U::Class c) const { return u().class_of(b) == c; }
  uint64_t tipval(int t) const { return H(1, (uint64_t)t, tipv[t], 0); }
  uint64_t def_value(const DevOp &d) const { return H(tipval(d.c1), tipval(d.c2), matv[d.pm1], matv[d.pm2]); }
  uint64_t memval(int c) const { return c < I->tips ? tipval(c) : dev[c]; }
  uint64_t refval(int c) const { return c < I->tips ? tipval(c) : ref[c]; }

  // what a buffer IS after a launch: device memory, or its definition over what its inputs are
  uint64_t value(int c, int depth = 0) const
  {
    if (c < I->tips) return tipval(c);
    if (!u().is_unstored(c)) return dev[c];
    if (depth > I->nbuf) die("definitions form a cycle", c);
    const DevOp &d = u().def(c);
    return H(value(d.c1, depth + 1), value(d.c2, depth + 1), matv[d.pm1], matv[d.pm2]);
  }

  [[noreturn]] void die(const char *what, int a = -1, int b = -1) const
  {
    fprintf(stderr, "UNSTORED_MODEL FAIL (class %d): %s (%d, %d) after %ld launches\n", cls, what, a, b, n_launch);
    exit(1);
  }

  // One launch.  Every queued operation carries its number in the upper bits of DevOp::pad (the library uses bits 0-2 and copies
  // the rest along), so the device's run of the REWRITTEN queue can be followed in lockstep with the plain semantics (every
  // operation stored, in queue order): `cur` is the plain value of every buffer at the point the device has reached.
  void launch(const EdgeEval *ee)
  {
    std::vector<uint64_t> cur = ref;
    size_t jp = 0;
    auto plain = [&](size_t upto) { // apply the queued operations jp .. upto - 1
      for (; jp < upto; ++jp)
      {
        const DevOp &o = queued[jp];
        const uint64_t v1 = o.c1 < I->tips ? tipval(o.c1) : cur[o.c1], v2 = o.c2 < I->tips ? tipval(o.c2) : cur[o.c2];
        cur[o.dest] = H(v1, v2, matv[o.pm1], matv[o.pm2]);
      }
    };
    rewrite_pending(I, ee, true);
    I->unstored.keep_clear(); // (as flush_impl does)
    const std::vector<DevOp> &L = I->pending;
    const bool has_inl = !I->pending_inl.empty();
    if (has_inl && I->pending_inl.size() != L.size()) die("pending_inl is not parallel to pending");
    // The step plan the record encoders will read (phyhip_step_plan.hpp), on the rewritten list, against this model's own
    // interpretation below: a child the plan takes from a register must be that register here, one it loads must not be stale
    // (said behind the model's own check of the value read, whose wording the controls know).
    // (Lists of one or two operations travel in the kernel arguments, unpadded: the plan is asked for as many records.)
    const int n_rec = L.size() >= 3 ? padded_records((int)L.size()) : (int)L.size();
    std::vector<StepPlan> plan((size_t)n_rec);
    plan_steps(L.data(), (int)L.size(), has_inl ? I->pending_inl.data() : (const InlineDef *)nullptr, I->tips, RegWindow{2}, kPadBits, n_rec, plan.data());
    auto against_plan = [&](size_t r, int s, int c, int bit, const DevOp &o, int m1, int m2) {
      const Reach got = plan[r].reach[s];
      const Reach own = (o.pad & bit) ? Reach::InStep : c < I->tips ? Reach::Tip : c == m1 ? Reach::Prev1 : c == m2 ? Reach::Prev2 : Reach::Loaded;
      if (got != own)
        die((got == Reach::Prev1 || got == Reach::Prev2) ? "the step plan forwards a child that is not the model's register"
                                                         : "the step plan and the model disagree on how a child reaches its step", c, (int)r);
      if (plan[r].stored != !(o.pad & 1) || plan[r].op != (int)std::min(r, L.size() - 1)) die("the step plan and the list disagree on a record's operation or store", o.dest, (int)r);
    };
    int      d1 = -1, d2 = -1; // destinations of the previous two operations
    uint64_t r1 = 0, r2 = 0;   // ... and their results (registers)
    for (size_t k = 0; k < L.size(); ++k)
    {
      const DevOp &o = L[k];
      const size_t tag = (size_t)((unsigned)o.pad >> 8);
      if ((o.pad & 6) && L.size() < 3) die("in-step child in a launch of the argument form", (int)k);
      if ((o.pad & 1) && L.size() < 3) die("non-storing operation in a launch of the argument form", (int)k);
      if (tag)
      { // a queued operation at its place: everything queued in front of it has happened in the plain semantics (also the
        // operations that left their place), it has not yet
        if (tag - 1 < jp || tag - 1 >= queued.size()) die("queued operations out of order", (int)k, (int)tag);
        plain(tag - 1);
      }
      else
      { // an operation the library put in: it belongs to the queued operation that follows it (a definition re-issued in front of
        // its reader: what left its place in front of that reader has happened), or to the end of the queue
        size_t nxt = 0;
        for (size_t j = k + 1; j < L.size() && !nxt; ++j) nxt = (size_t)((unsigned)L[j].pad >> 8);
        if (nxt && nxt - 1 < jp) die("queued operations out of order", (int)k, (int)nxt);
        plain(nxt ? nxt - 1 : queued.size());
      }
      auto child = [&](int c, int bit) -> uint64_t {
        uint64_t v;
        if (!(o.pad & bit) || has_inl) against_plan(k, bit == 4, c, bit, o, d1, d2);
        if (o.pad & bit)
        {
          if (!has_inl) die("in-step flag without a definition", (int)k);
          const InlineDef &d = I->pending_inl[k];
          if (d.a < 0 || d.a >= I->tips || d.b < 0 || d.b >= I->tips) die("in-step definition is not tip x tip", (int)k);
          ++n_instep;
          v = H(tipval(d.a), tipval(d.b), matv[d.pmA], matv[d.pmB]);
        }
        else if (c < I->tips) return tipval(c);
        else if (c == d1) v = r1;
        else if (c == d2) v = r2;
        else v = dev[c];
        if (v != cur[c]) die("an operation reads another value than the plain semantics hold at that point (stale memory, a stale register or a stale definition)", c, (int)k);
        if (plan[k].reach[bit == 4] == Reach::Loaded && dev[c] != cur[c]) die("the step plan loads a child that is stale in memory", c, (int)k);
        return v;
      };
      const uint64_t v = H(child(o.c1, 2), child(o.c2, 4), matv[o.pm1], matv[o.pm2]);
      if (tag) plain(tag); // (the operation itself)
      if (v != cur[o.dest]) die("an operation computes another value than the plain semantics hold for its buffer at that point", o.dest, (int)k);
      if (o.pad & 1) ++n_nostore;
      else dev[o.dest] = v;
      d2 = d1; r2 = r1; d1 = o.dest; r1 = v;
    }
    plain(queued.size());
    if ((L.size() & 1) && L.size() >= 3)
    { // The pipelined kernels alternate two register sets: an odd LIST (three operations or more; shorter ones travel in the kernel
      // arguments and are not padded) runs its last operation once more, one position later -- its own result is now the newest
      // register, the previous operation's the second, and what was two steps back is gone: read from memory
      const size_t k = L.size() - 1;
      const DevOp &o = L[k];
      ++n_pad;
      auto child = [&](int c, int bit) -> uint64_t {
        uint64_t v;
        against_plan(L.size(), bit == 4, c, bit, o, d1, d2); // (the pad's own record: d1 is the last operation's own result)
        if (o.pad & bit)
        {
          const InlineDef &d = I->pending_inl[k];
          v = H(tipval(d.a), tipval(d.b), matv[d.pmA], matv[d.pmB]);
        }
        else if (c < I->tips) return tipval(c);
        else if (c == d2) v = r2; // (the operation in front of the last one)
        else v = dev[c];
        if (v != cur[c]) die("the re-run of an odd list's last operation reads a stale value", c, (int)k);
        if (plan[L.size()].reach[bit == 4] == Reach::Loaded && dev[c] != cur[c]) die("the step plan's padded re-run loads a child that is stale in memory", c, (int)k);
        return v;
      };
      const uint64_t v = H(child(o.c1, 2), child(o.c2, 4), matv[o.pm1], matv[o.pm2]);
      if (v != cur[o.dest]) die("the re-run of an odd list's last operation computes another value", o.dest, (int)k);
      if (!(o.pad & 1)) dev[o.dest] = v;
      r1 = v;
    }
    if (ee)
      for (int side : {ee->parent, ee->child})
      {
        if (side < I->tips) continue;
        const uint64_t seen = (side == d1) ? r1 : dev[side];
        if (seen != cur[side]) die("the evaluation sees another value than the plain semantics", side);
      }
    std::vector<char> dest_now(I->nbuf, 0);
    for (const DevOp &o : queued) dest_now[o.dest] = 1;
    ref = cur;
    queued.clear();
    I->pending.clear();
    I->unstored.n_front = 0; // (as retire_queue does)
    std::fill(I->mat_in_queue.begin(), I->mat_in_queue.end(), 0);
    ++n_launch;
    check_after_launch(dest_now);
  }

  // memory and definitions after a launch
  void check_after_launch(const std::vector<char> &dest_now)
  {
    int n[4] = {0, 0, 0, 0};
    for (int b = I->tips; b < I->nbuf; ++b)
    {
      ++n[u().class_of(b)];
      if (u().class_of(b) > cls) die("a buffer is in a class that is switched off", b, u().class_of(b));
      if (is(b, U::kVirtual))
      {
        const DevOp &d = u().def(b);
        if (d.c1 >= I->tips || d.c2 >= I->tips) die("a virtual buffer's definition is not tip x tip", b);
        if (def_value(d) != ref[b]) die("a virtual buffer's definition is not its plain value", b);
      }
      else if ((cls < 2 || !u().is_unstored(b)) && written[b] && dev[b] != ref[b])
        die(cls < 2 ? "a buffer is neither stored nor virtual" : "a buffer is neither stored nor unstored", b);
    }
    for (U::Class c : {U::kVirtual, U::kDeferred, U::kChained})
      if (n[c] != u().n(c)) die("the count of a class does not count its buffers", (int)c, u().n(c));
    if (n[U::kVirtual] + n[U::kDeferred] + n[U::kChained] != u().n_unstored()) die("n_unstored does not count the unstored buffers");
    for (int b = I->tips; b < I->nbuf; ++b)
    {
      if (!is(b, U::kDeferred)) was_def[b] = 0;
      if (!u().is_unstored(b) || is(b, U::kVirtual)) continue;
      const DevOp &d = u().def(b);
      if (d.pad != 0) die(is(b, U::kDeferred) ? "a deferred definition carries flags" : "a chained definition carries flags", b);
      if (is(b, U::kDeferred))
        for (int c : {d.c1, d.c2})
          if (c >= I->tips && is(c, U::kVirtual)) die("a deferred definition reads a virtual buffer", b, c);
      if (cls < 3)
      { // (a deferred definition is one step over stored inputs, and stays so)
        for (int c : {d.c1, d.c2})
          if (c >= I->tips && u().is_unstored(c)) die("a deferred definition reads an unstored buffer", b, c);
        const bool fresh = !was_def[b] || dest_now[b] || memcmp(&seen_def[b], &d, sizeof d) != 0;
        if (fresh) { in1[b] = refval(d.c1); in2[b] = refval(d.c2); seen_def[b] = d; was_def[b] = 1; }
        if (memval(d.c1) != in1[b] || memval(d.c2) != in2[b]) die("a deferred definition's input is not in memory as it was when the definition was made", b);
        if (refval(d.c1) != in1[b] || refval(d.c2) != in2[b]) die("a deferred definition's input has another plain value than when the definition was made", b);
        if (H(in1[b], in2[b], matv[d.pm1], matv[d.pm2]) != ref[b]) die("a deferred definition is not its buffer's plain value", b);
        continue;
      }
      for (int c : {d.c1, d.c2})
      { // (a deferred definition is made over stored inputs; a list that chains may leave one of them chained behind it)
        if (c < I->tips) continue;
        if (u().is_unstored(c) ? u().seq(c) >= u().seq(b) : (!written[c] || dev[c] != ref[c]))
          die("a definition's input is neither stored nor unstored under an older sequence number", b, c);
      }
      if (is(b, U::kChained))
      {
        int len = 1; // (the longest chain of definitions that read buffers, ending in a chained one: a figure)
        for (int c = b;;)
        {
          const DevOp &e = u().def(c);
          auto link = [&](int x) { return x >= I->tips && (is(x, U::kChained) || is(x, U::kDeferred)); };
          const int nx = link(e.c1) ? e.c1 : link(e.c2) ? e.c2 : -1;
          if (nx < 0) break;
          c = nx; ++len;
        }
        max_chain = std::max(max_chain, (long)len);
      }
      if (value(b) != ref[b]) die("an unstored buffer's definition, evaluated over its inputs' definitions, is not its plain value", b);
    }
    const U::Counters &cd = u().counters(U::kDeferred), &cc = u().counters(U::kChained);
    if (cd.skipped != (unsigned long long)u().n(U::kDeferred) + cd.material + cd.dropped)
      die("deferred counters: deferred so far != deferred now + stored on demand + dropped");
    if (cc.skipped != (unsigned long long)u().n(U::kChained) + cc.material + cc.dropped)
      die("chained counters: chained so far != chained now + stored on demand + dropped");
  }
};

int main(int argc, char **argv)
{
  const int      cls = argc > 1 ? atoi(argv[1]) : 3;
  const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
  const int      events = argc > 3 ? atoi(argv[3]) : 2000, tips = argc > 4 ? atoi(argv[4]) : 12;
  const bool     soa = argc > 5 ? atoi(argv[5]) != 0 : true;
  const bool     in_step = argc > 6 ? atoi(argv[6]) != 0 : true; // 0: every virtual child re-issued as a step of its own (diag: PHYHIP_VIRT_INLINE=0)
  if (cls < 1 || cls > 3 || tips < 2) { fprintf(stderr, "usage: unstored_model <class 1|2|3> <seed> <events> <tips> <soa 0|1> [in-step 1|0]\n"); return 2; }
  std::mt19937   rng(seed);
  auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };

  Instance *I = new Instance();
  Unstored &u = I->unstored;
  I->tips = tips; I->nbuf = 3 * tips;
  I->nmat = cls >= 3 ? 4 * tips + 2 : 2 * tips; // (class 3: enough matrices for a post-order with one per edge)
  I->nmat_all = I->nmat + 2 * (I->nbuf - I->tips);
  I->S = soa ? 4 : 20; I->C = 4; I->soa = soa; I->perm = !soa; I->nt_groups = 2; I->prefetch_dist = 2;
  u.resize(I->nbuf);
  I->mat_in_queue.assign(I->nmat_all, 0);
  u.virt_min_ops = 3 + rnd(6);
  u.defer_stores = cls >= 2;
  u.chain_min_ops = cls >= 3 ? 3 + rnd(6) : 0;
  I->virt_inline = in_step;

  Model M;
  M.I = I; M.cls = cls;
  M.tipv.assign(tips, 1); M.matv.assign(I->nmat_all, 1);
  M.ref.assign(I->nbuf, 0); M.dev.assign(I->nbuf, 0); M.written.assign(I->nbuf, 0);
  M.was_def.assign(I->nbuf, 0); M.seen_def.assign(I->nbuf, DevOp{0, 0, 0, 0, 0, 0}); M.in1.assign(I->nbuf, 0); M.in2.assign(I->nbuf, 0);

  auto queue_op = [&](int dest, int c1, int c2, int pm1 = -1, int pm2 = -1) {
    DevOp o{dest, c1, c2, pm1 < 0 ? rnd(I->nmat) : pm1, pm2 < 0 ? rnd(I->nmat) : pm2, 0};
    M.queued.push_back(o);
    o.pad = (int)(M.queued.size() << 8); // (its number in this queue, above the library's bits)
    I->pending.push_back(o);
    I->mat_in_queue[o.pm1] = 1; I->mat_in_queue[o.pm2] = 1;
    M.written[dest] = 1;
  };
  auto any_child = [&](int not_this) {
    for (;;)
    {
      const int c = rnd(I->nbuf);
      if (c == not_this) continue;
      if (c >= tips && !M.written[c]) continue; // (never written: the reference would read garbage as well)
      return c;
    }
  };
  // a "traversal": cherries first, then operations that read earlier results -- the shape that leaves buffers virtual
  auto queue_traversal = [&](int n) {
    std::vector<int> made;
    for (int k = 0; k < n; ++k)
    {
      const int dest = tips + rnd(I->nbuf - tips);
      const int kind = rnd(4);
      // (an operation never reads its own destination: phyhip_update_partials refuses it)
      int from = made.empty() ? -1 : made[rnd((int)made.size())];
      if (from == dest) from = -1;
      if (kind == 0 || from < 0) queue_op(dest, rnd(tips), rnd(tips));
      else if (kind == 1) queue_op(dest, from, rnd(tips));
      else queue_op(dest, from, any_child(dest));
      if (std::find(made.begin(), made.end(), dest) == made.end()) made.push_back(dest);
    }
  };
  // A post-order over distinct buffers, as Post_Order_Lk emits one: every result is read once, mostly by one of the next two
  // operations.  Replayed, it rewrites inputs and buffers in the same order -- a repeated Lk(NULL).  Class 3: every edge has its
  // own matrix (a one-sided traversal, the lists that chain); below, matrices are drawn at random.
  std::vector<std::vector<DevOp>> orders;
  auto make_order = [&]() {
    std::vector<int> bufs;
    for (int b = tips; b < I->nbuf; ++b) bufs.push_back(b);
    std::shuffle(bufs.begin(), bufs.end(), rng);
    const int n = std::min((int)bufs.size(), 3 + rnd(2 * tips - 3 > 0 ? 2 * tips - 3 : 1));
    std::vector<DevOp> ops;
    std::vector<int>   open; // results nobody has read yet
    std::vector<int>   mats;
    if (cls >= 3)
    {
      for (int m = 0; m < I->nmat; ++m) mats.push_back(m);
      std::shuffle(mats.begin(), mats.end(), rng);
    }
    for (int k = 0; k < n; ++k)
    {
      auto take = [&](bool newest) {
        if (open.empty() || rnd(3) == 0) return rnd(tips);
        const size_t at = (newest || rnd(3)) ? open.size() - 1 : (size_t)rnd((int)open.size());
        const int    c = open[at];
        open.erase(open.begin() + (long)at);
        return c;
      };
      const int c1 = take(true), c2 = take(false);
      const int m1 = cls >= 3 ? mats[2 * k] : rnd(I->nmat), m2 = cls >= 3 ? mats[2 * k + 1] : rnd(I->nmat);
      ops.push_back(DevOp{bufs[k], c1, c2, m1, m2, 0});
      open.push_back(bufs[k]);
    }
    return ops;
  };
  if (cls >= 2)
    for (int k = 0; k < 3; ++k) orders.push_back(make_order());
  auto is = [&](int b, U::Class c) { return u.class_of(b) == c; };
  // a deferred or chained buffer -- class 3: one whose definition reads buffers; the ends of the chained definitions by sequence number
  auto any_dependant = [&]() {
    std::vector<int> d;
    for (int b = tips; b < I->nbuf; ++b)
      if ((is(b, U::kDeferred) || is(b, U::kChained)) && (cls < 3 || u.def(b).c1 >= tips || u.def(b).c2 >= tips)) d.push_back(b);
    return d.empty() ? -1 : d[rnd((int)d.size())];
  };
  auto chain_end = [&](bool last) {
    int e = -1;
    for (int b = tips; b < I->nbuf; ++b)
      if (is(b, U::kChained) && (e < 0 || (last ? u.seq(b) > u.seq(e) : u.seq(b) < u.seq(e)))) e = b;
    return e;
  };
  // phyhip_update_eigen_lr stores what its products read, rewrites the queue ONCE WITHOUT LAUNCHING (a short list: it decides on
  // the queue as it will be launched) and flushes afterwards, which rewrites it again: from class 3 the reader events do the same
  // half of the time
  long n_double = 0;
  auto reader = [&](int b) {
    devirtualise(I, b);
    if (cls >= 3 && rnd(2)) { rewrite_pending(I, nullptr, false); ++n_double; }
  };
  auto read_back = [&](int b, const char *what) {
    if (u.is_unstored(b) || M.dev[b] != M.ref[b]) M.die(what, b);
  };
  long n_input_writes = 0, n_replays = 0, n_mid_writes = 0, n_end_reads = 0;
  const int kinds = cls >= 3 ? 17 : cls == 2 ? 14 : 10; // (events 10-13: from class 2; 14-16: from class 3)
  for (int ev = 0; ev < events; ++ev)
  {
    switch (rnd(kinds))
    {
      case 10: case 11: case 14:
      { // a post-order traversal with its evaluation at the root, now and then a new one
        if (rnd(8) == 0) orders[rnd((int)orders.size())] = make_order();
        const std::vector<DevOp> &ops = orders[rnd((int)orders.size())];
        for (const DevOp &o : ops) queue_op(o.dest, o.c1, o.c2, o.pm1, o.pm2);
        ++n_replays;
        if (rnd(4))
        {
          EdgeEval ee{ops.back().dest, rnd(tips), rnd(I->nmat), nullptr, true, nullptr};
          M.launch(&ee);
        }
        else M.launch(nullptr);
        break;
      }
      case 12: case 13:
      { // a short list writes an input of a deferred or chained buffer (Update_Partial_Lk on the way of a search) -- a buffer in the
        // middle of a chain, when the input is chained itself; then a reader of the dependant
        const int b = any_dependant();
        if (b < 0) break;
        const DevOp d = u.def(b);
        const int   c = d.c1 >= tips ? d.c1 : d.c2;
        if (c < tips) break;
        M.launch(nullptr);
        if (!is(b, U::kDeferred) && !is(b, U::kChained)) break;
        const uint64_t old = M.ref[b];
        n_mid_writes += cls >= 3 && u.is_unstored(c);
        if (rnd(2)) queue_op(c, rnd(tips), rnd(tips));
        else
        {
          queue_op(c, any_child(c), rnd(tips));
          const int up = tips + rnd(I->nbuf - tips); // (... and the buffer above it, as the path of an SPR move does)
          if (up != c && rnd(2)) queue_op(up, c, rnd(tips));
        }
        ++n_input_writes;
        M.launch(nullptr);
        if (M.queued.empty() && M.ref[b] == old && rnd(2))
        {
          reader(b);
          M.launch(nullptr);
          if (u.is_unstored(b) || M.dev[b] != old)
            M.die(cls < 3 ? "a deferred buffer whose input was rewritten does not read back its old value"
                          : "an unstored buffer whose input was rewritten does not read back its old value", b, c);
        }
        break;
      }
      case 15: case 16:
      { // readers of a chain's two ends: the last buffer before any reader of the first (across launches), or both inside one queue
        // -- first then last (the last one's closure finds the first already queued), or last then first
        M.launch(nullptr);
        const int first = chain_end(false), last = chain_end(true);
        if (first < 0 || first == last) break;
        ++n_end_reads;
        switch (rnd(3))
        {
          case 0:
            reader(last); M.launch(nullptr); read_back(last, "a reader of a chain's last buffer finds it unstored or stale");
            reader(first); M.launch(nullptr); read_back(first, "a reader of a chain's first buffer, behind one of its last, finds it unstored or stale");
            break;
          case 1: reader(first); reader(last); M.launch(nullptr); break;
          default: reader(last); reader(first); M.launch(nullptr); break;
        }
        read_back(first, "a chain's first buffer does not read back");
        read_back(last, "a chain's last buffer does not read back");
        break;
      }
      case 0: case 1: queue_traversal(3 + rnd(14)); break;                       // a long list
      case 2: queue_traversal(1 + rnd(2)); break;                                // a short one
      case 3:
      { // an evaluation
        EdgeEval ee{any_child(-1), any_child(-1), rnd(I->nmat), nullptr, true, nullptr};
        M.launch(&ee);
        break;
      }
      case 4: M.launch(nullptr); break;                                          // a launch without an evaluation
      case 5:
      { // a reader of memory (phyhip_get_partials, Update_Eigen_Lr as its own kernel): the buffer is stored after the launch
        const int b = tips + rnd(I->nbuf - tips);
        if (!M.written[b]) break;
        reader(b);
        M.launch(nullptr);
        read_back(b, "a reader finds its buffer unstored or stale");
        break;
      }
      case 6:
      { // a matrix changes (store-first route): what is queued runs on the old value, dependants are stored on it
        const int m = rnd(I->nmat);
        M.launch(nullptr);
        devirtualise_matrix(I, m);
        M.launch(nullptr);
        for (int b = tips; b < I->nbuf; ++b)
          if (u.is_unstored(b) && (u.def(b).pm1 == m || u.def(b).pm2 == m)) M.die("an unstored buffer still reads a matrix that changes", b, m);
        ++M.matv[m];
        break;
      }
      case 7:
      { // a tip row changes
        const int t = rnd(tips);
        M.launch(nullptr);
        devirtualise_tip(I, t);
        M.launch(nullptr);
        for (int b = tips; b < I->nbuf; ++b)
          if (u.is_unstored(b) && (u.def(b).c1 == t || u.def(b).c2 == t)) M.die("an unstored buffer still reads a tip row that changes", b, t);
        ++M.tipv[t];
        break;
      }
      case 8:
        if (rnd(4) == 0)
        { // everything stored (phyhip_set_virtual_buffers(0) / another threshold)
          u.virt_min_ops = 0;
          devirtualise_all(I);
          M.launch(nullptr);
          if (u.n_unstored() != 0) M.die("devirtualise_all left unstored buffers");
          u.virt_min_ops = 1 + rnd(12);
          if (cls >= 3) u.chain_min_ops = rnd(5) ? 3 + rnd(10) : 0; // (the chained class has its own threshold; 0: off, what is chained stays until settled)
        }
        break;
      default: queue_traversal(6 + rnd(20)); break;
    }
  }
  M.launch(nullptr);
  const U::Counters &cv = u.counters(U::kVirtual), &cd = u.counters(U::kDeferred), &cc = u.counters(U::kChained);
  printf("UNSTORED_MODEL OK class %d seed %u: %ld launches, %llu stores skipped, %ld in-step children, %ld non-storing operations, %llu stored on demand, %ld odd lists re-ran their last operation, %llu stores deferred, %llu deferred stored on demand, %llu deferred dropped, %ld input writes, %ld replays, %llu stores chained, %llu chained stored on demand, %llu chained dropped, %ld longest chain, %ld writes under a chained input, %ld reads of chain ends, %ld queues rewritten twice\n",
         cls, seed, M.n_launch, cv.skipped, M.n_instep, M.n_nostore, cv.material, M.n_pad, cd.skipped, cd.material, cd.dropped, n_input_writes,
         n_replays, cc.skipped, cc.material, cc.dropped, M.max_chain, n_mid_writes, n_end_reads, n_double);
  delete I;
  return 0;
}
