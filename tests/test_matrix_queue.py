"""phyhip_matrix_queue.hpp, the one statement of "enqueue a matrix refresh, the last writer wins", of the snapshot slots and of
"forget the table", against a naive model: a map from matrix to (payload, slot) plus the list of matrices in insertion order.
A stand-alone C++ program that includes the header alone is compiled with the host compiler under the address and
undefined-behaviour sanitizers and run as a child process; it drives both payload types the library uses (double: the edge
length of a rebuild; const double *: an upload's staged copy) with seeded random sequences of put / put_if_absent /
want_snapshot / clear over 1, 3 and 70 matrices and checks the whole table after every step.  CPU-only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "phyhip_matrix_queue.hpp"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
using namespace phyhip_host;

static long g_steps = 0, g_checks = 0;
static void require(bool ok, const char *what, int nmat, long step)
{
  ++g_checks;
  if (ok) return;
  printf("FAIL %s at nmat %d step %ld\n", what, nmat, step);
  exit(1);
}

static double g_pool[256]; // (what the pointer payloads point at)
template <typename P> P make_payload(unsigned r);
template <> double make_payload<double>(unsigned r) { return 0.001 * (double)(r % 100000); }
template <> const double *make_payload<const double *>(unsigned r) { return &g_pool[r % 256]; }

template <typename P> struct Model
{
  std::map<int, std::pair<P, int>> entry; // matrix -> (payload, snapshot slot)
  std::vector<int>                 order; // matrices in order of first insertion
};

// the whole table against the model
template <typename P> void check(const MatrixTable<P> &t, const Model<P> &m, int nmat, long step)
{
  const size_t n = m.order.size();
  require(t.size() == n && t.idx().size() == n && t.payload().size() == n && t.snapshot().size() == n, "the arrays are parallel", nmat, step);
  require(t.empty() == (n == 0), "empty()", nmat, step);
  int snaps = 0;
  for (size_t k = 0; k < n; ++k)
  {
    const auto &e = m.entry.at(m.order[k]);
    require(t.idx()[k] == m.order[k], "first-insertion order", nmat, step);
    require(t.payload()[k] == e.first, "an entry's payload is the last one put", nmat, step);
    require(t.snapshot()[k] == e.second, "an entry's snapshot slot", nmat, step);
    require(t.queued(t.idx()[k]), "the reverse map knows a queued matrix", nmat, step);
    snaps += t.snapshot()[k] != -1;
  }
  int queued = 0;
  for (int x = 0; x < nmat; ++x)
  {
    require(t.queued(x) == (m.entry.count(x) != 0), "the reverse map agrees with the arrays", nmat, step);
    queued += t.queued(x);
  }
  require((size_t)queued == n, "one entry per queued matrix", nmat, step);
  require(t.snapshots() == snaps, "snapshots() counts the slots that are not -1", nmat, step);
}

template <typename P> void put(MatrixTable<P> &t, Model<P> &m, int x, P v, bool if_absent, int nmat, long step)
{
  const bool   was = m.entry.count(x) != 0;
  const size_t n0 = t.size();
  if (if_absent) require(t.put_if_absent(x, v) == !was, "put_if_absent says whether it queued", nmat, step);
  else t.put(x, v);
  if (!was) { m.entry[x] = {v, -1}; m.order.push_back(x); }
  else if (!if_absent) m.entry[x].first = v; // (the payload only: place and snapshot slot stay)
  require(t.size() == n0 + !was, "a queued matrix is not appended again", nmat, step);
  check(t, m, nmat, step);
}

template <typename P> void clear(MatrixTable<P> &t, Model<P> &m, int nmat, long step)
{
  t.clear();
  m.entry.clear(); m.order.clear();
  check(t, m, nmat, step);
  require(t.size() == 0 && t.snapshots() == 0, "cleared: sizes and count 0", nmat, step);
  for (int x = 0; x < nmat; ++x) require(!t.queued(x), "cleared: nothing queued", nmat, step);
}

template <typename P> void random_run(int nmat, unsigned seed, long steps)
{
  std::mt19937   rng(seed);
  MatrixTable<P> t;
  Model<P>       m;
  t.reset(nmat);
  check(t, m, nmat, -1);
  bool cleared = false;
  for (long s = 0; s < steps; ++s, ++g_steps)
  {
    const unsigned r = rng() % 100;
    const int      x = (int)(rng() % (unsigned)nmat);
    if (r < 45) put(t, m, x, make_payload<P>(rng()), false, nmat, s);
    else if (r < 65) put(t, m, x, make_payload<P>(rng()), true, nmat, s);
    else if (r < 92)
    { // a snapshot slot for a queued matrix that has none (what matrices_touch grants)
      if (!m.entry.count(x) || m.entry[x].second != -1) continue;
      const int slot = nmat + (int)(rng() % 1000);
      t.want_snapshot(x, slot);
      m.entry[x].second = slot;
      check(t, m, nmat, s);
    }
    else
    {
      clear(t, m, nmat, s);
      cleared = true;
      if (rng() % 3 == 0) clear(t, m, nmat, s); // twice in a row
      if (rng() % 2)
      { // the put that follows starts at position 0
        put(t, m, x, make_payload<P>(rng()), false, nmat, s);
        require(t.size() == 1 && t.idx()[0] == x && t.snapshot()[0] == -1, "after clear() a put starts at position 0", nmat, s);
      }
    }
  }
  require(cleared, "the run cleared at least once", nmat, steps);
}

// 65 puts of distinct matrices (past 4 * kUploadBatch = 64, where the library flushes uploads by itself), a snapshot for every
// third, each payload overwritten once; then two clears in a row and a table that starts again
template <typename P> void long_run()
{
  const int      nmat = 70;
  MatrixTable<P> t;
  Model<P>       m;
  t.reset(nmat);
  for (int k = 0; k < 65; ++k)
  {
    const int x = (k * 37 + 11) % nmat; // (37 and 70 are coprime: distinct)
    put(t, m, x, make_payload<P>((unsigned)k), false, nmat, k);
    if (k % 3 == 0) { t.want_snapshot(x, nmat + k); m.entry[x].second = nmat + k; check(t, m, nmat, k); }
  }
  require(t.size() == 65 && t.snapshots() == 22, "65 distinct matrices, 22 snapshots", nmat, 65);
  for (int k = 0; k < 65; ++k) put(t, m, (k * 37 + 11) % nmat, make_payload<P>(1000u + (unsigned)k), k % 2 != 0, nmat, 65 + k);
  require(t.size() == 65 && t.snapshots() == 22, "overwriting appends nothing and keeps the snapshots", nmat, 130);
  clear(t, m, nmat, 131);
  clear(t, m, nmat, 132);
  put(t, m, 69, make_payload<P>(7u), true, nmat, 133);
  require(t.size() == 1 && t.idx()[0] == 69 && t.snapshots() == 0, "after two clears a put starts at position 0", nmat, 133);
  t.reset(3); // (reset: an empty table over another range)
  m.entry.clear(); m.order.clear();
  check(t, m, 3, 134);
}

int main()
{
  const int nmats[] = {1, 3, 70};
  for (int nmat : nmats)
    for (unsigned seed = 1; seed <= 4; ++seed)
    {
      random_run<double>(nmat, seed, 4000);
      random_run<const double *>(nmat, 100 + seed, 4000);
    }
  long_run<double>();
  long_run<const double *>();
  printf("steps %ld checks %ld\ndone\n", g_steps, g_checks);
  return 0;
}
"""


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    d = tmp_path_factory.mktemp("matrix_queue")
    src, exe = d / "queue.cpp", d / "queue"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "phyml_amd", "csrc"), str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.split("\n")
    assert lines[-2] == "done"
    words = lines[-3].split()
    return {words[0]: int(words[1]), words[2]: int(words[3])}


def test_the_tables_follow_the_naive_model_under_both_sanitizers(figures):
    # (the fixture asserts the program's exit status: every `require` of it held, for both payload types, after every step)
    assert figures["steps"] == 3 * 4 * 2 * 4000
    assert figures["checks"] > figures["steps"]


def test_the_header_is_plain_host_code_and_keeps_its_inline_functions_hidden():
    text = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_matrix_queue.hpp")).read()
    assert "__global__" not in text and "__device__" not in text and "#include <hip" not in text and '#include "' not in text
    assert text.count("#pragma GCC visibility push(hidden)") == 1 and text.count("#pragma GCC visibility pop") == 1
