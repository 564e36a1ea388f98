"""phyhip_step_plan.hpp, the one statement of "the results of the last operations are still in registers", against a naive model
that replays the padded list step by step and keeps nothing but the destinations of the last two steps: no positions, no
distances.  A stand-alone C++ program that includes the header alone is compiled with the host compiler under the address and
undefined-behaviour sanitizers and run as a child process.  Inputs: seeded random post-orders over 3 to 40 tips -- odd and even
lengths, in-step children, non-storing re-issues in front of their readers, an operation that reads its own destination (the
entry points refuse one; the rule is by buffer index and the pad's first register is only reached that way) -- and hand lists of
one and two operations, each at window depths 0, 1 and 2.  The writer-side questions the planner of unstored buffers asks are
checked against the same replay.  The program counts what it met and fails unless every reach occurred in both child positions
at every depth that allows it and the padded re-run read a child from memory and from each register level; two controls -- the
window without the pad's shift, a depth-2 plan handed to a depth-1 consumer -- must fail.  CPU-only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_step_plan.hpp")

PROGRAM = r"""
#include "phyhip_step_plan.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
using namespace phyhip_host;

struct Op { int dest, c1, c2, pad; };   // (anything with these fields: the header is a template over it)
struct Def { int a, b; };
static const PadBits kBits{1, {2, 4}};
enum Control { kNone, kNoPadShift, kDepthMismatch };
static Control g_control = kNone;

static long g_lists = 0, g_records = 0, g_checks = 0;
static long g_seen[3][2][5], g_pad_seen[3][5]; // [depth][child][reach], [depth][reach] of the padded re-run's children
static long g_unstorable = 0, g_pad_rule = 0;  // writer-side answers that were "yes"

[[noreturn]] static void fail(const char *what, int depth, int at, int s)
{
  printf("FAIL %s (depth %d, position %d, child %d) in list %ld\n", what, depth, at, s, g_lists);
  exit(1);
}

// The naive model: run the padded list, remember the destinations of the last two steps
static void naive(const std::vector<Op> &L, const Def *defs, int tips, int depth, int n_rec, std::vector<StepPlan> &out)
{
  int d1 = -1, d2 = -1;
  out.resize((size_t)n_rec);
  for (int r = 0; r < n_rec; ++r)
  {
    const int op = std::min(r, (int)L.size() - 1); // (behind the list: its last operation once more)
    const Op &o = L[(size_t)op];
    for (int s = 0; s < 2; ++s)
    {
      const int c = s ? o.c2 : o.c1;
      Reach x = Reach::Loaded;
      if (defs && (o.pad & (s ? 4 : 2))) x = Reach::InStep;
      else if (c < tips) x = Reach::Tip;
      else if (depth >= 1 && c == d1) x = Reach::Prev1;
      else if (depth >= 2 && c == d2) x = Reach::Prev2;
      out[(size_t)r].reach[s] = x;
    }
    out[(size_t)r].op = op;
    out[(size_t)r].stored = !(o.pad & 1);
    d2 = d1; d1 = o.dest;
  }
}

static void check_list(const std::vector<Op> &L, const std::vector<Def> &D, int tips, int n_rec)
{
  const int  n = (int)L.size();
  const Def *defs = D.empty() ? nullptr : D.data();
  ++g_lists;
  for (int depth = 0; depth <= 2; ++depth)
  {
    const RegWindow win{depth};
    std::vector<StepPlan> want, got((size_t)n_rec);
    naive(L, defs, tips, g_control == kDepthMismatch && depth == 2 ? 1 : depth, n_rec, want);
    if (g_control == kNoPadShift && n_rec > n)
    { // the pad planned at its operation's own position
      plan_steps(L.data(), n, defs, tips, win, kBits, n, got.data());
      got[(size_t)n] = got[(size_t)n - 1];
    }
    else plan_steps(L.data(), n, defs, tips, win, kBits, n_rec, got.data());
    for (int r = 0; r < n_rec; ++r, ++g_records)
    {
      ++g_checks;
      if (got[(size_t)r].op != want[(size_t)r].op) fail("a record stands for another operation", depth, r, -1);
      if (got[(size_t)r].stored != want[(size_t)r].stored) fail("a record's store", depth, r, -1);
      for (int s = 0; s < 2; ++s)
      {
        if (got[(size_t)r].reach[s] != want[(size_t)r].reach[s]) fail("how a child reaches its step", depth, r, s);
        ++g_seen[depth][s][(int)got[(size_t)r].reach[s]];
        if (r == n) ++g_pad_seen[depth][(int)got[(size_t)r].reach[s]];
      }
    }
    if (n_rec != padded_records(n)) continue; // (records in the kernel arguments, unpadded: no writer-side question)
    // The writer's side, for results written once in the list: every read stays in registers <=> somebody behind reads it, and the
    // LAST reader of the buffer finds it in a register in the replay; the pad reads it from memory <=> the replay's pad loads it
    std::vector<int> n_dest((size_t)(4 * tips + 8), 0), last_read((size_t)(4 * tips + 8), -1);
    for (int k = 0; k < n; ++k)
    {
      ++n_dest[(size_t)L[(size_t)k].dest];
      if (L[(size_t)k].c1 >= tips && !(L[(size_t)k].pad & 2)) last_read[(size_t)L[(size_t)k].c1] = k;
      if (L[(size_t)k].c2 >= tips && !(L[(size_t)k].pad & 4)) last_read[(size_t)L[(size_t)k].c2] = k;
    }
    for (int w = 0; w < n; ++w)
    {
      const int b = L[(size_t)w].dest, lr = last_read[(size_t)b];
      if (n_dest[(size_t)b] != 1) continue;
      bool in_regs = false;
      if (lr > w)
        for (int s = 0; s < 2; ++s)
          if ((s ? L[(size_t)lr].c2 : L[(size_t)lr].c1) == b && !(L[(size_t)lr].pad & (s ? 4 : 2)))
            in_regs = want[(size_t)lr].reach[s] == Reach::Prev1 || want[(size_t)lr].reach[s] == Reach::Prev2;
      ++g_checks;
      if (reads_stay_in_registers(win, w, lr) != in_regs) fail("every read of a result falls inside the window", depth, w, -1);
      g_unstorable += in_regs;
      bool pad_loads = false;
      if (n & 1)
        for (int s = 0; s < 2; ++s)
          if ((s ? L[(size_t)n - 1].c2 : L[(size_t)n - 1].c1) == b && want[(size_t)n].reach[s] == Reach::Loaded) pad_loads = true;
      ++g_checks;
      if (pad_reads_from_memory(win, L.data(), n, w) != pad_loads) fail("the padded re-run reads a result from memory", depth, w, -1);
      g_pad_rule += pad_loads;
    }
  }
}

// A post-order as a traversal emits one: every result is read once, mostly by one of the next two operations.  Buffers tips ..
// 2 tips - 2 are results, 2 tips .. 3 tips - 1 virtual ones (written by nothing but a re-issue, or read in-step).
static void random_list(std::mt19937 &rng, int tips, bool in_step, bool reissues, bool self_read)
{
  auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
  std::vector<Op>  L;
  std::vector<Def> D;
  std::vector<int> open;
  const int n_ops = 3 + rnd(tips - 2), virt0 = 2 * tips;
  int       next_virt = 0;
  for (int k = 0; k < n_ops; ++k)
  {
    auto take = [&](bool newest) {
      if (open.empty() || rnd(3) == 0) return rnd(tips);
      const size_t at = (newest || rnd(3)) ? open.size() - 1 : (size_t)rnd((int)open.size());
      const int    c = open[at];
      open.erase(open.begin() + (long)at);
      return c;
    };
    Op  o{tips + k, take(true), take(false), rnd(4) == 0 ? 1 : 0};
    Def d{-1, -1};
    for (int s = 0; s < 2; ++s)
    { // a tip child becomes a virtual buffer: computed in-step, or re-issued in front (not storing) and forwarded
      int &c = s ? o.c2 : o.c1;
      if (c >= tips || rnd(4) || next_virt >= tips) continue;
      const int v = virt0 + next_virt++;
      if (in_step && d.a < 0 && rnd(2)) { c = v; o.pad |= s ? 4 : 2; d = Def{rnd(tips), rnd(tips)}; }
      else if (reissues) { c = v; L.push_back(Op{v, rnd(tips), rnd(tips), 1}); D.push_back(Def{-1, -1}); }
    }
    L.push_back(o); D.push_back(d);
    open.push_back(o.dest);
  }
  if (self_read)
  { // (never through an in-step child: such a child's index is a virtual buffer's, which no operation of the list writes)
    const int s = rnd(2);
    (s ? L.back().c2 : L.back().c1) = L.back().dest;
    L.back().pad &= ~(s ? 4 : 2);
  }
  if (!in_step) D.clear();
  check_list(L, D, tips, padded_records((int)L.size()));
}

int main(int argc, char **argv)
{
  if (argc > 1) g_control = !strcmp(argv[1], "no_pad_shift") ? kNoPadShift : !strcmp(argv[1], "depth_mismatch") ? kDepthMismatch : kNone;
  // hand lists of one and two operations over 3 tips, in a device slot (padded) and in the kernel arguments (as many records)
  const Op one[] = {{3, 0, 1, 0}, {3, 0, 1, 1}, {3, 4, 1, 0}, {3, 3, 4, 0}};
  for (const Op &o : one)
    for (int n_rec : {1, 2}) check_list({o}, {}, 3, n_rec);
  const Op two[][2] = {{{3, 0, 1, 0}, {4, 3, 2, 0}}, {{3, 0, 1, 1}, {4, 2, 3, 0}}, {{3, 0, 1, 0}, {4, 5, 3, 0}}, {{3, 0, 1, 0}, {4, 3, 3, 0}},
                       {{3, 0, 1, 0}, {3, 4, 2, 0}}};
  for (const auto &t : two) check_list({t[0], t[1]}, {}, 3, 2);
  check_list({{3, 6, 1, 2}, {4, 3, 7, 4}}, {{0, 1}, {2, 0}}, 3, 2); // (in-step children in both positions)
  std::mt19937 rng(20240611u);
  for (int tips = 3; tips <= 40; ++tips)
    for (int rep = 0; rep < 24; ++rep) random_list(rng, tips, rep & 1, rep & 2, rep % 6 == 5);
  for (int depth = 0; depth <= 2; ++depth)
  {
    for (int s = 0; s < 2; ++s)
      for (int x = 0; x < 5; ++x)
      {
        const bool allowed = !((x == (int)Reach::Prev1 && depth < 1) || (x == (int)Reach::Prev2 && depth < 2));
        if (allowed != (g_seen[depth][s][x] > 0)) fail(allowed ? "a reach never occurred" : "a reach occurred beyond the window", depth, x, s);
      }
    if (!g_pad_seen[depth][(int)Reach::Loaded] || (depth >= 1) != (g_pad_seen[depth][(int)Reach::Prev1] > 0) ||
        (depth >= 2) != (g_pad_seen[depth][(int)Reach::Prev2] > 0))
      fail("the padded re-run did not read a child from memory and from each register level", depth, -1, -1);
  }
  if (!g_unstorable || !g_pad_rule) fail("a writer-side question was never answered yes", -1, -1, -1);
  printf("lists %ld records %ld checks %ld unstorable %ld pad_rule %ld\n", g_lists, g_records, g_checks, g_unstorable, g_pad_rule);
  for (int depth = 0; depth <= 2; ++depth)
    for (int s = 0; s < 2; ++s)
      printf("seen depth %d child %d: %ld %ld %ld %ld %ld\n", depth, s, g_seen[depth][s][0], g_seen[depth][s][1], g_seen[depth][s][2],
             g_seen[depth][s][3], g_seen[depth][s][4]);
  for (int depth = 0; depth <= 2; ++depth)
    printf("pad depth %d: %ld %ld %ld %ld %ld\n", depth, g_pad_seen[depth][0], g_pad_seen[depth][1], g_pad_seen[depth][2], g_pad_seen[depth][3],
           g_pad_seen[depth][4]);
  printf("done\n");
  return 0;
}
"""

REACHES = ("Tip", "Prev1", "Prev2", "InStep", "Loaded")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)])
    return str(exe)


def run(exe, *args):
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_the_plan_follows_the_naive_replay_under_both_sanitizers(program):
    r = run(program)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "done"
    head = lines[0].split()
    fig = {head[k]: int(head[k + 1]) for k in range(0, len(head), 2)}
    assert fig["lists"] == 4 * 2 + 5 + 1 + 38 * 24 and fig["records"] > 3 * 2 * fig["lists"] and fig["checks"] > fig["records"]
    assert fig["unstorable"] > 0 and fig["pad_rule"] > 0
    # (the program refuses to finish otherwise; said again here, from its figures)
    seen = {}
    for ln in lines:
        if ln.startswith("seen depth"):
            w = ln.replace(":", "").split()
            seen[(int(w[2]), int(w[4]))] = dict(zip(REACHES, map(int, w[5:])))
        if ln.startswith("pad depth"):
            w = ln.replace(":", "").split()
            seen[("pad", int(w[2]))] = dict(zip(REACHES, map(int, w[3:])))
    for depth in (0, 1, 2):
        for child in (0, 1):
            for name, n in seen[(depth, child)].items():
                allowed = not ((name == "Prev1" and depth < 1) or (name == "Prev2" and depth < 2))
                assert (n > 0) == allowed, (depth, child, name, n)
        pad = seen[("pad", depth)]
        assert pad["Loaded"] > 0 and (pad["Prev1"] > 0) == (depth >= 1) and (pad["Prev2"] > 0) == (depth >= 2), (depth, pad)


@pytest.mark.parametrize("control, what", (("no_pad_shift", "how a child reaches its step"), ("depth_mismatch", "how a child reaches its step")))
def test_a_control_fails(program, control, what):
    """the window without the pad's shift; a depth-2 plan handed to a consumer whose kernel forwards one step"""
    r = run(program, control)
    assert r.returncode == 1 and ("FAIL " + what) in r.stdout and "done" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_host_code_and_keeps_its_inline_functions_hidden():
    text = open(HEADER).read()
    assert "__global__" not in text and "__device__" not in text and "#include <hip" not in text and '#include "' not in text
    assert text.count("#pragma GCC visibility push(hidden)") == 1 and text.count("#pragma GCC visibility pop") == 1
