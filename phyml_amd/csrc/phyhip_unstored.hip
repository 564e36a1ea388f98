// phyhip_unstored.hip -- the buffers a launch leaves unstored (virtual, deferred, chained: Unstored, phyhip_host.hpp): which results
// of a queue stay in registers, what is stored in front of a queue that needs them, and the queue as it will be launched
// (libphyhip.so, host code only -- no kernel lives here; the units and what they share: phyhip_host.hpp)
#include "phyhip_host.hpp"
#include <algorithm>

namespace phyhip_host
{
using U = Unstored;

// The launch in between must leave the buffer in memory, whatever the queue does with it (rewrite_pending)
static void keep_stored(Instance *I, int buf)
{
  if (buf >= I->tips && buf < I->nbuf && I->unstored.virt_min_ops > 0)
    I->unstored.keep(buf);
}

// The storing definition of one unstored buffer into the front of the queue.  A virtual definition reads tips, a deferred one
// tips and buffers that have not been written since (rewrite_pending stores or drops it before one is); such a buffer may be
// unstored itself -- under a chained definition, and under a deferred one made by a list that chains (defer_forwarded's second pass) -- and then
// its definition goes in first, transitively.  The definitions in front of the queue stay in ascending order of their sequence
// numbers, so one queued by an earlier call that reads a buffer stored by this one still finds it written in front of it.
static void store_definition(Instance *I, int buf)
{
  Unstored   &u  = I->unstored;
  const DevOp op = u.def(buf);
  if (u.class_of(buf) != U::kVirtual && u.n(U::kChained) > 0) // (a deferred definition's inputs were stored when it was made; a list that chains may have left one unstored behind it)
    for (int c : {op.c1, op.c2})
      if (c >= I->tips && u.is_unstored(c))
      { // (stored for good, like the buffer that was asked for: whoever asked may be about to change a tip row or a matrix under it)
        keep_stored(I, c);
        store_definition(I, c);
      }
  size_t at = 0;
  u.n_front = std::min(u.n_front, (int)I->pending.size());
  while (at < (size_t)u.n_front && u.seq(I->pending[at].dest) < u.seq(buf)) ++at;
  ++u.n_front;
  I->pending.insert(I->pending.begin() + (long)at, op);
  mark_matrix_readers(I, op.pm1, op.pm2);
  u.end(buf, U::kMaterial);
}

void devirtualise(Instance *I, int buf)
{
  // whoever asks is about to read the buffer from memory -- a kernel outside the traversal launch (eigen_lr_kernel, a mixture
  // combination), a copy to the host, or a setter that changes what the buffer was computed from: the launch in between must not
  // leave it virtual AGAIN (a long queue that writes it with a tip x tip operation and reads it later would: rewrite_pending)
  keep_stored(I, buf);
  if (buf < I->tips || buf >= I->nbuf || !I->unstored.is_unstored(buf)) return;
  store_definition(I, buf);
}

// devirtualise every unstored buffer whose definition `reads` (a scan of the class bytes: only while there are some)
template <typename F> static void devirtualise_where(Instance *I, F &&reads)
{
  const Unstored &u = I->unstored;
  for (int b = I->tips; b < I->nbuf && u.n_unstored() > 0; ++b)
    if (u.is_unstored(b) && reads(u.class_of(b), u.def(b))) devirtualise(I, b);
}
void devirtualise_all(Instance *I) { devirtualise_where(I, [](U::Class, const DevOp &) { return true; }); }
void devirtualise_matrix(Instance *I, int m) { devirtualise_where(I, [m](U::Class, const DevOp &d) { return d.pm1 == m || d.pm2 == m; }); }
void devirtualise_tip(Instance *I, int tip) { devirtualise_where(I, [tip](U::Class, const DevOp &d) { return d.c1 == tip || d.c2 == tip; }); }
// A buffer is about to be written by something that does not pass through the queue (a setter): deferred and chained buffers whose
// definitions read it are stored first, on its old value (their own dependants then read them from memory)
void devirtualise_dependants(Instance *I, int buf)
{
  if (buf < I->tips) return;
  devirtualise_where(I, [buf](U::Class c, const DevOp &d) { return c != U::kVirtual && (d.c1 == buf || d.c2 == buf); });
}

// Where settle_deferred's scan of the queue starts.  The stored definitions already standing in front (the first n_front entries)
// write values their dependants are defined on -- making an input real does not invalidate a dependant -- so while a chained
// definition exists the scan starts behind them: from 0, a deferred dependant of a chain whose last definition has just been
// stored in front would count as "input written" and be stored too.  With no chained definition about no definition reads an
// unstored buffer, and the scan covers the whole queue as it always did.
static int settle_scan_start(const Unstored &u, int n0) { return u.n(U::kChained) > 0 ? std::min(u.n_front, n0) : 0; }

// Deferred and chained buffers left by earlier launches against the list that is about to run and its evaluation, in order: one
// rule for both classes.  For the definition d of b -- needed: b is read before it is written; dead: b is written before it is read
// (every repeated whole-tree traversal ends here for every such buffer: two scans of the list, nothing launched).  M0 = {needed} +
// {not dead, and the list writes one of d's input buffers: stored in front, where d still reads the input's old value}; M = M0
// closed under "unstored input of a member" (store_definition's recursion).  M is stored in front, in sequence order; dead
// definitions outside M are dropped; the rest stays.  A kept definition cannot have a dropped input: the list writes that input,
// which puts the dependant into M0.  (A dead input in M is stored and overwritten later.)  Returns whether it stored one (a short
// launch then stores them all: it is a list now in any case, and the short launches behind it keep their form).
static bool settle_deferred(Instance *I, const EdgeEval *ee)
{
  Unstored &u = I->unstored;
  if (u.n(U::kDeferred) == 0 && u.n(U::kChained) == 0) return false;
  const int        n0 = (int)I->pending.size(), never = n0 + 1;
  std::vector<int> first_read(I->nbuf, never), first_write(I->nbuf, never);
  for (int k = settle_scan_start(u, n0); k < n0; ++k)
  {
    const DevOp &o = I->pending[k];
    for (int c : {o.c1, o.c2})
      if (c >= I->tips && first_read[c] == never) first_read[c] = k;
    if (first_write[o.dest] == never) first_write[o.dest] = k;
  }
  if (ee)
    for (int c : {ee->parent, ee->child})
      if (c >= I->tips && first_read[c] == never) first_read[c] = n0;
  auto written = [&](int c) { return c >= I->tips && first_write[c] != never; };
  auto settles = [&](int b) { return u.is_unstored(b) && u.class_of(b) != U::kVirtual; };
  const unsigned long long before = u.n_material();
  std::vector<int>         m0;
  for (int b = I->tips; b < I->nbuf; ++b)
  {
    if (!settles(b)) continue;
    const bool needed = first_read[b] < first_write[b], dead = !needed && first_write[b] != never;
    if (needed || (!dead && (written(u.def(b).c1) || written(u.def(b).c2)))) m0.push_back(b);
  }
  for (int b : m0)
    if (u.is_unstored(b)) devirtualise(I, b); // (an earlier member's closure may have stored it)
  for (int b = I->tips; b < I->nbuf && u.n(U::kDeferred) + u.n(U::kChained) > 0; ++b)
    if (settles(b) && first_write[b] != never) u.end(b, U::kDropped); // (what is still unstored is not needed: dead)
  return u.n_material() != before;
}

// Does the list qualify for the chained class?  At least chain_min_ops operations, virtual buffers on, and no transition matrix
// read twice (one-sided traversals: in a both-sided one the post-order and the pre-order share the edge matrices, and each refresh
// of one would store whole closures -- matrices_touch).
static bool list_chains(const Instance *I, const std::vector<DevOp> &L, const std::vector<InlineDef> &LI)
{
  const int n = (int)L.size();
  if (I->unstored.chain_min_ops <= 0 || n < I->unstored.chain_min_ops || I->unstored.virt_min_ops <= 0) return false;
  std::vector<unsigned char> seen(I->mat_in_queue.size(), 0);
  auto twice = [&](int m) { if (m < 0) return false; if (seen[m]) return true; seen[m] = 1; return false; };
  for (int k = 0; k < n; ++k)
  {
    if (twice(L[k].pm1) || twice(L[k].pm2)) return false;
    if ((L[k].pad & (kOpInl1 | kOpInl2)) && (twice(LI[k].pmA) || twice(LI[k].pmB))) return false;
  }
  return true;
}

// Deferred buffers, the rule (on the list as it will be launched, front to back): a storing operation whose destination is written
// once in the list, read in it only inside the kernel's register window (`win`; phyhip_step_plan.hpp: the reads the step plan
// calls Prev1 / Prev2) and neither read by the evaluation nor asked for from memory (keep_real) does not store, if each child is a tip or a buffer that is
// in memory after this launch: not virtual, not computed in-step, not deferred, not written again behind the operation.  So every
// deferred definition is made as ONE step over stored inputs, and in a list that does not chain it stays so: no recursion and no
// order among definitions.
// Chained buffers (`chain`: list_chains), a second pass with the same conditions over what the first left storing, but for the
// children: a child may be a tip or ANY buffer that is not written again behind the operation.  It is then either in memory
// after this launch, or unstored under a definition that computes the value this operation read -- virtual (read in-step or
// through a re-issue; a list writes a buffer it leaves virtual once), deferred, or chained earlier in this list.  In such a list a
// result deferred by the first pass may see one of its stored inputs chained by the second (it is one of that input's two readers):
// then the deferred definition reads an unstored buffer too, and its sequence number is renewed so that the definitions of the
// list are numbered in list order, inputs before dependants (store_definition follows the inputs of both classes).
static void defer_forwarded(Instance *I, const EdgeEval *ee, std::vector<DevOp> &L, bool chain, RegWindow win)
{
  Unstored        &u = I->unstored;
  const int        n = (int)L.size();
  std::vector<int> n_dest(I->nbuf, 0), last_write(I->nbuf, -1), last_read(I->nbuf, -1);
  for (int k = 0; k < n; ++k)
  {
    const DevOp &o = L[k];
    ++n_dest[o.dest];
    last_write[o.dest] = k;
    if (o.c1 >= I->tips && !(o.pad & kOpInl1)) last_read[o.c1] = k;
    if (o.c2 >= I->tips && !(o.pad & kOpInl2)) last_read[o.c2] = k;
  }
  auto in_memory = [&](int c, bool in_step, int i) {
    return c < I->tips || (!in_step && u.class_of(c) != U::kVirtual && u.class_of(c) != U::kDeferred && last_write[c] < i);
  };
  auto not_rewritten = [&](int c, int i) { return c < I->tips || last_write[c] < i; };
  for (int pass = 0; pass < (chain ? 2 : 1); ++pass)
    for (int i = 0; i + 1 < n; ++i)
    {
      DevOp &o = L[i];
      if (pass == 1 && (o.pad & kOpNoStore) && u.class_of(o.dest) == U::kDeferred) u.renew(o.dest); // (deferred by pass 0)
      if ((o.pad & kOpNoStore) || n_dest[o.dest] != 1) continue;
      if (!reads_stay_in_registers(win, i, last_read[o.dest])) continue; // (never read behind it, or read from memory)
      if ((ee && (ee->parent == o.dest || ee->child == o.dest)) || u.kept(o.dest)) continue;
      if (pass == 0 && (!in_memory(o.c1, o.pad & kOpInl1, i) || !in_memory(o.c2, o.pad & kOpInl2, i))) continue;
      if (pass == 1 && (!not_rewritten(o.c1, i) || !not_rewritten(o.c2, i))) continue;
      if (pad_reads_from_memory(win, L.data(), n, i)) continue; // (the odd-list rule, for this class)
      u.make(pass == 0 ? U::kDeferred : U::kChained, o.dest, o);
      o.pad |= kOpNoStore;
    }
}

// The queue as it will be launched.  Short lists (or kernels without two-deep forwarding): the first one that reads a virtual
// buffer gets the storing definitions of ALL virtual buffers in front of it.  Long lists (a window of depth 2): a tip x tip operation
// whose result is written once in this list, read only later in it and not by the evaluation leaves its place; every reader of a
// virtual buffer -- one left virtual by this list or by an earlier one -- computes it inside its own step (one per operation:
// DevOp::pad bits 1-2, pending_inl) or gets the definition re-issued in front of it, not storing (the kernels forward the
// results of the previous two operations in registers); what the evaluation edge reads is stored.
void rewrite_pending(Instance *I, const EdgeEval *ee, RegWindow forwarding)
{
  Unstored &u = I->unstored;
  I->pending_inl.clear();
  const bool stored_deferred = settle_deferred(I, ee);
  const int  n0 = (int)I->pending.size();
  auto is_virtual = [&](int b) { return b >= I->tips && u.class_of(b) == U::kVirtual; };
  // (only launches of the LIST form: one- and two-operation launches -- records in the kernel arguments, the resident evaluators --
  // run kernels without in-step children and without the second forwarding level's guarantees: a list must keep three
  // operations even if each of its tip x tip operations leaves its place)
  // (depth 2: two non-storing re-issues in front of one reader lean on the second forwarding level)
  bool virtualise = forwarding.depth == 2 && u.virt_min_ops > 0 && n0 >= u.virt_min_ops && n0 >= 3;
  if (virtualise)
  {
    int stay = 0;
    for (const DevOp &o : I->pending) stay += !(o.c1 < I->tips && o.c2 < I->tips);
    virtualise = stay >= 3;
  }
  if (!virtualise && u.n_unstored() == 0) return;
  if (!virtualise)
  { // A short launch.  If it reads a virtual buffer, EVERY virtual buffer is stored now, in this one launch: the short launches
    // of a tree search (SPR candidates, Lk(b), Br_Len_Opt) come in long runs after a full traversal, and one list of tip x tip
    // operations in front of the first of them costs less than a launch of three operations -- instead of a resident command
    // -- at each buffer's first use.
    bool reads = false;
    for (const DevOp &o : I->pending) reads = reads || is_virtual(o.c1) || is_virtual(o.c2);
    if (ee) reads = reads || is_virtual(ee->parent) || is_virtual(ee->child);
    if (reads || stored_deferred) devirtualise_all(I); // (deferred buffers go with them; and with one that settle_deferred had to store)
    // (a queued operation that WRITES a virtual buffer stores it: real again -- its old definition must never be stored over it)
    for (const DevOp &o : I->pending)
      if (is_virtual(o.dest)) u.end(o.dest, U::kShortLaunch);
    return;
  }
  std::vector<unsigned char> skip;
  {
    std::vector<int> n_dest(I->nbuf, 0), first_read(I->nbuf, -1);
    for (int k = 0; k < n0; ++k)
    {
      const DevOp &o = I->pending[k];
      ++n_dest[o.dest];
      for (int c : {o.c1, o.c2})
        if (c >= I->tips && first_read[c] < 0) first_read[c] = k;
    }
    skip.assign(n0, 0);
    for (int k = 0; k < n0; ++k)
    {
      const DevOp &o = I->pending[k];
      if (o.c1 < I->tips && o.c2 < I->tips && n_dest[o.dest] == 1 && first_read[o.dest] > k &&
          !(ee && (ee->parent == o.dest || ee->child == o.dest)) && !u.kept(o.dest))
        skip[k] = 1;
    }
  }
  std::vector<DevOp>     L;
  std::vector<InlineDef> LI; // (parallel to L)
  L.reserve((size_t)n0 + (size_t)u.n(U::kVirtual) + 8);
  LI.reserve(L.capacity());
  const InlineDef none{-1, -1, -1, -1};
  // both pipelined kernels compute ONE virtual child inside its reader's step (phyhip_nt2.hpp / phyhip_aa.hpp, INL); a second
  // one is re-issued as a non-storing operation in front of the reader
  const bool in_step = I->virt_inline && ((I->soa && I->nt_groups <= 2) || I->perm); // (the instantiations that exist: flush_impl)
  bool       any_inl = false;
  auto before_read = [&](int c, DevOp &reader, InlineDef &rin, int bit) {
    if (!is_virtual(c)) return;
    DevOp d = u.def(c);
    mark_matrix_readers(I, d.pm1, d.pm2);
    ++u.n_recomputed;
    if (in_step && rin.a < 0 && reader.c1 != reader.c2)
    {
      rin = InlineDef{d.c1, d.c2, d.pm1, d.pm2};
      reader.pad |= bit;
      any_inl = true;
      return;
    }
    d.pad = kOpNoStore;
    L.push_back(d); LI.push_back(none);
  };
  for (int k = 0; k < n0; ++k)
  {
    DevOp o = I->pending[k];
    if (skip[k])
    { // from here on the buffer is what this operation says; nothing is launched for it until somebody reads it
      if (is_virtual(o.dest)) u.end(o.dest, U::kOverwritten);
      u.make(U::kVirtual, o.dest, o);
      continue;
    }
    InlineDef in = none;
    before_read(o.c1, o, in, kOpInl1);
    if (o.c2 != o.c1) before_read(o.c2, o, in, kOpInl2);
    L.push_back(o); LI.push_back(in);
    if (is_virtual(o.dest)) u.end(o.dest, U::kOverwritten); // (a storing operation: the buffer is real again)
  }
  auto store_now = [&](int b) { // what is read from memory behind this launch (or by its evaluation): stored
    if (!is_virtual(b)) return;
    const DevOp d = u.def(b);
    u.end(b, U::kMaterial);
    mark_matrix_readers(I, d.pm1, d.pm2);
    L.push_back(d); LI.push_back(none);
  };
  for (int b : u.keep_real) store_now(b);
  if (ee)
    for (int side : {ee->parent, ee->child}) store_now(side);
  // The pipelined kernels pad an odd list by running its last operation once more (phyhip_step_plan.hpp), at a position where the
  // result at the far end of the last operation's window is no longer in registers: a child of the last operation produced there
  // is then read from memory -- so it must have been stored (two non-storing re-issues in front of a reader; reachable without
  // in-step children)
  if (const int far = (int)L.size() - 1 - forwarding.depth; far >= 0)
  {
    DevOp &d1 = L[far];
    if ((d1.pad & kOpNoStore) && pad_reads_from_memory(forwarding, L.data(), (int)L.size(), far))
    {
      d1.pad &= ~kOpNoStore;
      if (is_virtual(d1.dest)) u.end(d1.dest, U::kMaterial);
    }
  }
  if (u.defer_stores) defer_forwarded(I, ee, L, list_chains(I, L, LI), forwarding);
  I->pending.swap(L);
  if (any_inl) I->pending_inl.swap(LI);
  // (the rewritten list is launched as it stands: flush_impl.  A SHORT list leaves here as it came, its stored definitions still
  // in front and n_front still counting them -- phyhip_update_eigen_lr rewrites its queue once without launching and the flush
  // rewrites it again: the second settle_deferred must still know them, and a definition stored then must still find its place)
  u.n_front = 0;
}

} // namespace phyhip_host
