"""phyhip_scan_plan.hpp, the one statement of the candidate-list calls' chunk arithmetic and work-space layouts, against the
bindings' independent restatement (capi.*_chunk_candidates), and its distinct-length slot table.  A stand-alone C++ program that
includes the header alone is compiled with the host compiler under the address and undefined-behaviour sanitizers and run as a
child process: it checks the layouts' regions (stated order, contiguous, total == fixed + chunk * per, the triple's 256-byte
boundary) and the slot table itself, and prints chunk, fixed and per over a grid of shapes and bounds.  CPU-only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = 128 << 20

PROGRAM = r"""
#include "phyhip_scan_plan.hpp"
#include <cstdio>
#include <cstdlib>
using namespace phyhip_host;

static void require(bool ok, const char *what, size_t P, size_t S, size_t M, size_t chunk)
{
  if (ok) return;
  printf("FAIL %s at P %zu S %zu M %zu chunk %zu\n", what, P, S, M, chunk);
  exit(1);
}

// every region starts where the one before it ends, in the stated order
static void check_scan(size_t P, size_t S, size_t M, size_t classes, size_t c)
{
  const ScanLayout L(P, S, M, classes, c);
  const size_t     pe = (P + 1) / 2 * 2, tiles = (P + 255) / 256, vecs = classes ? classes : 1;
  const size_t     start[] = {L.keep, L.exps, L.mats, L.tile_sums, L.flags(c), L.sums(c), L.prefix, L.recs, L.lengths(c), L.total};
  const size_t     size[] = {P * M * S * 8, vecs * pe * 4, 3 * c * M * S * S * 8, c * tiles * 8, c * 8, c * 8, classes ? 200 + 128 * classes : 0,
                             c * 32, 3 * c * 8};
  require(L.keep == 0, "scan: the kept vector is first", P, S, M, c);
  for (int i = 0; i < 9; ++i) require(start[i + 1] == start[i] + size[i], "scan: regions in order, none overlapping", P, S, M, c);
  require(L.total == L.fixed + c * L.per, "scan: total == fixed + chunk * per", P, S, M, c);
  require(L.keep_of(vecs - 1) + P * (classes ? 1 : M) * S * 8 == L.exps && L.exps_of(vecs - 1) + pe * 4 == L.mats, "scan: the last kept vector", P, S, M, c);
  require(L.matrix(3 * c - 1, classes ? classes - 1 : 0) + (classes ? 1 : M) * S * S * 8 == L.tile_sums, "scan: the last matrix", P, S, M, c);
  for (size_t n = 1; n <= c && n <= 3; ++n) // a shorter launch packs its flags and sums behind its own tile sums
    require(L.flags(n) == L.tile_sums + n * tiles * 8 && L.sums(n) == L.flags(n) + n * 8 && L.sums(n) + n * 8 <= L.prefix && L.lengths(n) + 3 * n * 8 <= L.total,
            "scan: a launch of n", P, S, M, c);
}

static void check_triple(size_t P, size_t S, size_t C, size_t c)
{
  const TripleLayout L(P, S, C, c);
  const size_t       pe = (P + 1) / 2 * 2, kept_end = L.exps + 3 * pe * 4;
  require(L.keep == 0 && L.exps == 3 * P * C * S * 8 && L.keep_of(2) + P * C * S * 8 == L.exps && L.exps_of(2) + pe * 4 == kept_end, "triple: the kept vectors", P, S, C, c);
  require(L.mats % 256 == 0 && L.mats >= kept_end && L.mats - kept_end < 256 && L.mats == L.fixed, "triple: the 256-byte boundary", P, S, C, c);
  const size_t start[] = {L.mats, L.dot, L.fact, L.recs, L.out, L.total};
  const size_t size[] = {3 * c * C * S * S * 8, c * P * C * S * 8, c * pe * 4, c * 40, c * 96};
  for (int i = 0; i < 5; ++i) require(start[i + 1] == start[i] + size[i], "triple: regions in order, none overlapping", P, S, C, c);
  require(L.total == L.fixed + c * L.per, "triple: total == fixed + chunk * per", P, S, C, c);
}

static double from_bits(unsigned long long b)
{
  double d;
  memcpy(&d, &b, sizeof d);
  return d;
}

int main()
{
  const size_t Ps[] = {1, 255, 256, 257, 300}, Ss[] = {4, 20}, Ms[2][3] = {{1, 4, 8}, {1, 4, 64}};
  const size_t huge = (size_t)-1;
  for (size_t P : Ps)
    for (size_t S : Ss)
      for (int kind = 0; kind < 3; ++kind) // plain scan, mixture scan, triple
        for (size_t M : Ms[kind == 1])
        {
          const size_t     classes = kind == 1 ? M : 0;
          const ScanLayout s(P, S, M, classes, 0);
          const TripleLayout t(P, S, M, 0);
          const size_t     fixed = kind == 2 ? t.fixed : s.fixed, per = kind == 2 ? t.per : s.per;
          const size_t     bounds[] = {1, fixed + per - 1, fixed + per, fixed + 12 * per, fixed + 12 * per + per / 2, (size_t)128 << 20};
          for (size_t b : bounds)
          {
            const size_t cap = kind == 2 ? huge : kScanGridCap, chunk = kind == 2 ? scan_chunk(b, fixed, per, huge) : scan_chunk(b, fixed, per, huge, cap);
            printf("%s %zu %zu %zu %zu %zu %zu %zu\n", kind == 0 ? "scan" : kind == 1 ? "mixture" : "triple", P, S, M, b, chunk, fixed, per);
            if (kind == 2) check_triple(P, S, M, chunk);
            else check_scan(P, S, M, classes, chunk);
            // the list is shorter than the bound allows
            require(scan_chunk(b, fixed, per, 1, cap) == 1 && (chunk == 1 || scan_chunk(b, fixed, per, chunk - 1, cap) == chunk - 1),
                    "the minimum with the list's length", P, S, M, chunk);
          }
        }

  SlotTable t;
  const double nan_a = from_bits(0x7ff8000000000000ull), nan_b = from_bits(0x7ff8000000000001ull);
  const double in[] = {0.5, 0.25, 0.5, 0.0, -0.0, nan_a, nan_a, nan_b};
  const int    want[] = {0, 1, 0, 2, 3, 4, 4, 5};
  for (int i = 0; i < 8; ++i) require(t.slot(in[i]) == want[i], "slot table: first-seen order by bits", (size_t)i, 0, 0, 0);
  require(t.lengths.size() == 6 && t.lengths[1] == 0.25, "slot table: one length per slot", 0, 0, 0, 0);
  t.reset();
  require(t.slot(0.25) == 0 && t.lengths.size() == 1, "slot table: reset", 0, 0, 0, 0);
  phyhip_regraft_candidate c = {7, 8, 9, PHYHIP_REGRAFT_SUBTREE_IS_LEFT, 0.1, 0.25, 0.1};
  const RegraftRec r = regraft_pack(c, t);
  require(r.c1 == 7 && r.c2 == 8 && r.sub == 9 && r.flags == PHYHIP_REGRAFT_SUBTREE_IS_LEFT && r.m1 == 1 && r.m2 == 0 && r.m3 == 1 && r.pad == 0,
          "record packing", 0, 0, 0, 0);
  printf("done\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "phyml_amd", "csrc"), str(src), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.split("\n")
    assert lines[-2] == "done"
    return [(ln.split()[0],) + tuple(int(x) for x in ln.split()[1:]) for ln in lines[:-2]]


def test_the_program_checked_its_layouts_and_the_slot_table(rows):
    # (the fixture asserts the program's exit status: every `require` of it held, under both sanitizers)
    assert len(rows) == 5 * 2 * 3 * 3 * 6
    assert {r[0] for r in rows} == {"scan", "mixture", "triple"}


def test_chunk_sizes_equal_the_bindings_restatement(rows):
    from phyml_amd import capi
    restated = {"scan": capi.regraft_chunk_candidates, "mixture": capi.mixture_regraft_chunk_candidates, "triple": capi.triple_chunk_candidates}
    for kind, P, S, M, bound, chunk, fixed, per in rows:
        assert restated[kind](P, M, S, bound) == chunk, (kind, P, S, M, bound, fixed, per)
        # the bounds around the first and the thirteenth candidate
        if bound in (1, fixed + per - 1, fixed + per):
            assert chunk == 1
        elif bound in (fixed + 12 * per, fixed + 12 * per + per // 2):
            assert chunk == 12


def test_the_default_bound_meets_the_grid_cap_only_in_the_scans(rows):
    at_default = {r[0]: r[5] for r in rows if r[1:5] == (1, 4, 1, DEFAULT)}
    assert at_default["scan"] == 65535 and at_default["mixture"] == 65535
    assert at_default["triple"] > 65535
