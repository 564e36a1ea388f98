// phyhip_matrix_queue.hpp -- the refreshes of transition matrices that wait for their launch (MatrixTable: device rebuilds from
// an edge length, phyhip_update_transition_matrices; uploads of host-computed matrices, phyhip_set_transition_matrix).  The ONE statement of
// "enqueue, last writer wins" and of "forget the table"; who flushes what and when: phyhip.hip, phyhip_queue.hip.
// Plain host C++: no HIP, no Instance -- a host compiler builds it alone (tests/test_matrix_queue.py).
#pragma once
#include <cassert>
#include <cstddef>
#include <vector>

#pragma GCC visibility push(hidden) // (inline functions of this header stay out of the library's dynamic symbols)
namespace phyhip_host
{

// One table of queued refreshes: per entry {matrix, payload, snapshot slot or -1} in three parallel, contiguous arrays in order of
// first insertion (the flushes copy or walk them as they stand), the reverse map matrix -> entry, and the number of entries that
// ask for a snapshot.  Payload: the edge length of a rebuild, or an upload's copy in pinned staging memory.
// A snapshot slot receives the matrix's OLD value before the refresh lands: the definition of an unstored buffer reads it there
// from then on (phyhip_host.hpp: Unstored; who grants one: matrices_touch).
template <typename Payload> struct MatrixTable
{
  void reset(int nmat) // an empty table over matrices 0 .. nmat - 1
  {
    clear();
    pos_.assign((size_t)nmat, -1);
  }
  bool   queued(int m) const { return pos_[m] >= 0; }
  size_t size() const { return idx_.size(); }
  bool   empty() const { return idx_.empty(); }
  int    snapshots() const { return n_snap_; } // entries whose snapshot slot is not -1
  const std::vector<int>     &idx() const { return idx_; }
  const std::vector<Payload> &payload() const { return val_; }
  const std::vector<int>     &snapshot() const { return snap_; }

  // the last writer wins: a queued matrix keeps its place and its snapshot slot and takes the new payload
  void put(int m, Payload v)
  {
    if (pos_[m] >= 0) { val_[pos_[m]] = v; return; }
    pos_[m] = (int)idx_.size();
    idx_.push_back(m); val_.push_back(v); snap_.push_back(-1);
  }
  // the first writer wins (a command nobody answered goes back behind what was queued since: requeue_sent)
  bool put_if_absent(int m, Payload v)
  {
    if (pos_[m] >= 0) return false;
    put(m, v);
    return true;
  }
  // An entry receives at most one snapshot slot between two clears -- matrices_touch stores the buffer instead of granting a
  // second -- so the count is exactly the number of entries with one.
  void want_snapshot(int m, int slot)
  {
    assert(pos_[m] >= 0 && slot >= 0 && snap_[pos_[m]] < 0);
    snap_[pos_[m]] = slot;
    ++n_snap_;
  }
  // the only way a table is emptied
  void clear()
  {
    for (int m : idx_) pos_[m] = -1;
    idx_.clear(); val_.clear(); snap_.clear();
    n_snap_ = 0;
  }

 private:
  std::vector<int>     idx_;  // queued matrices
  std::vector<Payload> val_;
  std::vector<int>     snap_; // per entry: the slot that receives the matrix's old value first, or -1
  std::vector<int>     pos_;  // matrix -> entry, or -1
  int                  n_snap_ = 0;
};

} // namespace phyhip_host
#pragma GCC visibility pop
