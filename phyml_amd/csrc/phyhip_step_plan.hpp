// phyhip_step_plan.hpp -- how each child of each step of a launch reaches it: the ONE statement of "the results of the last
// operations are still in registers".  The pipelined kernels forward the results of the previous one or two steps in registers
// (DESIGN section 4); what follows from it -- no load for such a child, no store for a result read only that way, memory left
// stale -- is decided from this header by everyone who decides it: the record encoders and the traffic count (phyhip_queue.hip)
// from plan_steps, the planner of unstored buffers (phyhip_unstored.hip) from the two writer-side questions below.
// Plain host C++: no HIP, no Instance -- a host compiler builds it alone (tests/test_step_plan.py).  Op: anything with the
// fields dest, c1, c2, pad of a queued operation (DevOp, phyhip_kernels.hpp).
#pragma once

#pragma GCC visibility push(hidden) // (inline functions of this header stay out of the library's dynamic symbols)
namespace phyhip_host
{

// How a child reaches its step: a tip row, the result of the step one or two positions in front (in registers), a virtual
// tip x tip result computed inside the step itself, or a load from memory.
enum class Reach : unsigned char { Tip, Prev1, Prev2, InStep, Loaded };

// The kernels alternate two register sets, so a list of n_ops operations runs as n_ops + (n_ops & 1) records: record r < n_ops
// is operation r, and the record at n_ops -- an odd list's pad -- runs the last operation once more (idempotent: same inputs,
// same output, same address), ONE POSITION LATER.  Positions in this padded list are what the window is defined on.
inline int padded_records(int n_ops) { return n_ops + (n_ops & 1); }
inline int op_of_record(int r, int n_ops) { return r < n_ops ? r : n_ops - 1; }

// The register window of a kernel: how many steps back a result is still in registers.  0: the kernels that read DevOps, and the
// records of a command for the large-grid evaluator (its two operations run one after the other per tile); 1 / 2: the pipelined
// kernels with loads one / two operations ahead.
struct RegWindow
{
  int depth;
  // is the result written at list position w in registers for the reader at padded position r?  (The pad sits at n_ops: the last
  // operation's own destination is one step back for it, and what the last operation found two steps back is three back -- gone.)
  bool holds(int w, int r) const { return r - w >= 1 && r - w <= depth; }
};

// DevOp::pad as the plan reads it: the bit of a result that is not stored, the bits of a child computed in-step
struct PadBits
{
  int no_store, in_step[2];
};

// One record of the launch: the operation it stands for, how its two children reach it, whether its result is stored
struct StepPlan
{
  int   op;
  Reach reach[2];
  bool  stored;
};

// The plan of a launch, n_rec = padded_records(n_ops) entries into `out` (the caller's: nothing is allocated here).  in_step: the
// in-step definitions parallel to ops, or nullptr -- the list has none, and no operation's in-step bits are set.  A child matches
// a register by its buffer index, the nearer register first, exactly as the kernels' flag bits say it.
template <typename Op, typename Def>
inline void plan_steps(const Op *ops, int n_ops, const Def *in_step, int tips, RegWindow win, PadBits bits, int n_rec, StepPlan *out)
{
  for (int r = 0; r < n_rec; ++r)
  {
    StepPlan &p = out[r];
    p.op = op_of_record(r, n_ops);
    const Op &o = ops[p.op];
    p.stored = !(o.pad & bits.no_store);
    for (int s = 0; s < 2; ++s)
    {
      const int c = s ? o.c2 : o.c1;
      if (in_step && (o.pad & bits.in_step[s])) p.reach[s] = Reach::InStep;
      else if (c < tips) p.reach[s] = Reach::Tip;
      else if (r >= 1 && win.holds(r - 1, r) && c == ops[r - 1].dest) p.reach[s] = Reach::Prev1;
      else if (r >= 2 && win.holds(r - 2, r) && c == ops[r - 2].dest) p.reach[s] = Reach::Prev2;
      else p.reach[s] = Reach::Loaded;
    }
  }
}

// The step's kind (kRecKindShift, phyhip_kernels.hpp: the straight-line bodies of the lane-per-pattern list kernel) from the plan:
// [child 1][child 2] over {a tip, the previous step's result, an in-step child} -> kind; 0 = the generic step.  rows_onehot[s]: every
// tip row child s reads (its own, or its in-step definition's two) is one-hot throughout.
inline unsigned kind_of(const StepPlan &p, const bool rows_onehot[2])
{
  static const unsigned char kinds[3][3] = {{0, 1, 6}, {2, 0, 4}, {5, 3, 0}};
  int how[2];
  for (int s = 0; s < 2; ++s)
    how[s] = (p.reach[s] == Reach::Tip && rows_onehot[s]) ? 0 : p.reach[s] == Reach::Prev1 ? 1 : (p.reach[s] == Reach::InStep && rows_onehot[s]) ? 2 : -1;
  return (how[0] >= 0 && how[1] >= 0) ? kinds[how[0]][how[1]] : 0u;
}

// ---- the writer's side: may the result written at list position w go unstored? ---------------------------------------------
// Every read of it in the list falls inside the window (last_read: the last list position that reads the buffer; none behind w, or
// one further back than the window: read from memory)
inline bool reads_stay_in_registers(RegWindow win, int w, int last_read) { return last_read > w && win.holds(w, last_read); }

// The padded re-run of an odd list's last operation reads it from memory: the last operation has it as a child, and at the pad's
// position it is no longer in registers, whatever the last operation itself found.  (By buffer index: the index of an in-step
// child is a virtual buffer's, which no operation of the list writes.)
template <typename Op> inline bool pad_reads_from_memory(RegWindow win, const Op *ops, int n_ops, int w)
{
  if (!(n_ops & 1)) return false;
  const Op &last = ops[n_ops - 1];
  return (last.c1 == ops[w].dest || last.c2 == ops[w].dest) && !win.holds(w, n_ops);
}

} // namespace phyhip_host
#pragma GCC visibility pop
