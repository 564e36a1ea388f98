// phyhip_scan_plan.hpp -- the planning of the calls that take a list of K candidates and run it in chunks under a work-space bound
// (phyhip_regraft.hip: the plain and the mixture regraft scan; phyhip_triple.hip: Triple_Dist; phyhip_pars.hip: the parsimony
// regraft scan, whose chunks are bounded by the grid alone): how many candidates a chunk holds,
// where every region of the work space lies, which matrix slot a length of the chunk gets, and the record a scan kernel reads.
// The ONE statement of those layouts: the runs place their device pointers with it, the getters read through the layout the run
// left on the unit (phyhip_side.hpp), and capi.*_chunk_candidates restates its sizes (tests/test_scan_plan.py holds the two equal).
// Plain host C++: no HIP, no Instance -- a host compiler builds it alone.  The driver that runs a plan: phyhip_scan.hpp.
#pragma once
#include "../../include/phyhip.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <unordered_map>
#include <vector>

#pragma GCC visibility push(hidden) // (inline functions of this header stay out of the library's dynamic symbols)
namespace phyhip_host
{

constexpr int    kRegraftTile = 256;      // patterns of a scan kernel's workgroup: a candidate has one partial sum per tile
constexpr size_t kScanGridCap = 65535;    // a grid's second dimension holds 65535 candidates
constexpr size_t kMixRegraftHeadBytes = 200, kMixRegraftClassBytes = 128; // sizeof(MixRegraftHead), sizeof(MixRegraftClass) (phyhip_regraft.hip)

// what a scan kernel reads of one candidate
struct RegraftRec
{
  int c1, c2, sub, flags; // partials buffer or tip index of the two children and the subtree; PHYHIP_REGRAFT_*
  int m1, m2, m3, pad;    // the three matrices: slots of the chunk's matrix area
};

// candidates per chunk: what the bound leaves behind the part every call reserves, at least one, no more than the list or the cap
inline size_t scan_chunk(size_t max_bytes, size_t fixed, size_t per, size_t count, size_t cap = (size_t)-1)
{
  const size_t chunk = max_bytes > fixed + per ? (max_bytes - fixed) / per : 1;
  return std::min(chunk, std::min(count, cap));
}

inline size_t scan_exponent_ints(size_t P) { return (P + 1) & ~(size_t)1; } // a vector's P exponents, rounded up to 8 bytes

// The work space of a regraft scan, byte offsets:
//   kept vector(s) | exponents | matrices | tile sums, flags, sums | (mixture: head, class table) | records | lengths
// plain scan: one kept vector [P][C][S] and its exponents, M = C matrices a slot, classes = 0;
// mixture:    per class a kept vector [P][S] and its exponents, M = classes matrices a slot, the head and the per-class table in
//             front of the records (`fixed` counts them: they are there whatever the chunk).
// A launch of n <= chunk candidates packs its flags (8 bytes a candidate) and sums right behind its n * tiles tile sums, so that
// what comes down is one copy; what goes up -- (head, table,) records, lengths -- is one copy too.
struct ScanLayout
{
  size_t tiles = 0, chunk = 0, exp_ints = 0, vec_bytes = 0, slot_bytes = 0, mat_bytes = 0; // (vec: one kept vector; slot: M matrices)
  size_t keep = 0, exps = 0, mats = 0, tile_sums = 0, prefix = 0, recs = 0;
  size_t prefix_bytes = 0, total = 0, fixed = 0, per = 0;
  ScanLayout(size_t P = 0, size_t S = 0, size_t M = 0, size_t classes = 0, size_t chunk_ = 0) : chunk(chunk_)
  {
    const size_t vecs = classes ? classes : 1;
    tiles = (P + kRegraftTile - 1) / kRegraftTile;
    exp_ints = scan_exponent_ints(P);
    vec_bytes = P * (classes ? 1 : M) * S * sizeof(double);
    mat_bytes = S * S * sizeof(double);
    slot_bytes = M * mat_bytes;
    prefix_bytes = classes ? kMixRegraftHeadBytes + classes * kMixRegraftClassBytes : 0;
    exps = keep + vecs * vec_bytes;
    mats = exps + vecs * exp_ints * sizeof(int);
    tile_sums = mats + 3 * chunk * slot_bytes;
    prefix = sums(chunk) + chunk * sizeof(double);
    recs = prefix + prefix_bytes;
    total = lengths(chunk) + 3 * chunk * sizeof(double);
    fixed = mats + prefix_bytes;
    per = 3 * slot_bytes + tiles * sizeof(double) + 8 + sizeof(double) + sizeof(RegraftRec) + 3 * sizeof(double);
  }
  size_t flags(size_t n) const { return tile_sums + n * tiles * sizeof(double); } // of a launch of n candidates
  size_t sums(size_t n) const { return flags(n) + n * 8; }
  size_t lengths(size_t n) const { return recs + n * sizeof(RegraftRec); }
  size_t keep_of(size_t cls) const { return keep + cls * vec_bytes; }
  size_t exps_of(size_t cls) const { return exps + cls * exp_ints * sizeof(int); }
  size_t matrix(size_t slot, size_t cls) const { return mats + slot * slot_bytes + cls * mat_bytes; } // (plain scan: cls 0, C matrices from there)
};

// The work space of phyhip_optimise_triples, byte offsets:
//   three kept vectors [P][C][S] | their exponents | (rounded up to 256 bytes: what lies behind is read as double2)
//   matrices | products | exponents | records | results
struct TripleLayout
{
  size_t chunk = 0, exp_ints = 0, vec_bytes = 0;
  size_t keep = 0, exps = 0, mats = 0, dot = 0, fact = 0, recs = 0, out = 0;
  size_t total = 0, fixed = 0, per = 0;
  TripleLayout(size_t P = 0, size_t S = 0, size_t C = 0, size_t chunk_ = 0) : chunk(chunk_)
  {
    exp_ints = scan_exponent_ints(P);
    vec_bytes = P * C * S * sizeof(double);
    exps = keep + 3 * vec_bytes;
    fixed = (exps + 3 * exp_ints * sizeof(int) + 255) & ~(size_t)255;
    mats = fixed;
    dot = mats + chunk * 3 * C * S * S * sizeof(double);
    fact = dot + chunk * vec_bytes;
    recs = fact + chunk * exp_ints * sizeof(int);
    out = recs + chunk * sizeof(phyhip_triple_candidate);
    total = out + chunk * sizeof(phyhip_triple_result);
    per = 3 * C * S * S * sizeof(double) + vec_bytes + exp_ints * sizeof(int) + sizeof(phyhip_triple_candidate) + sizeof(phyhip_triple_result);
  }
  size_t keep_of(size_t which) const { return keep + which * vec_bytes; }
  size_t exps_of(size_t which) const { return exps + which * exp_ints * sizeof(int); }
};

// The work space of phyhip_calculate_regraft_parsimony, byte offsets:
//   kept plane (Fitch: int2 [Pp]; step matrix: int [S][Pp]) | kept site scores int [Pp] | records | sums | tile sums
// Pp: the pattern count rounded up to even, as the planes of phyhip_pars.hip.  A candidate costs its 16-byte record, its 8-byte
// sum and 8 bytes per tile of 256 patterns (3 KB at 100 000 patterns), so the only bound on a chunk is the cap.
#ifndef PHYHIP_PARS_SLAB_FACTOR
#define PHYHIP_PARS_SLAB_FACTOR 8 // (measured against 4 and 16 with builds that define it otherwise: profiles/parsimony_regraft_scan.md)
#endif
constexpr int kParsScanSlabFactor = PHYHIP_PARS_SLAB_FACTOR; // slabs of a launch: enough for this many workgroups per compute unit (phyhip_pars.hip)
struct ParsScanRec
{
  int c1, c2, sub, flags; // plane or tip index of the two children and the subtree; bit 0: the subtree of the slab's previous record
};
struct ParsScanLayout
{
  size_t chunk = 0, Pp = 0, plane_bytes = 0, site_bytes = 0;
  size_t keep = 0, site = 0, recs = 0, sums = 0, tile_sums = 0, total = 0;
  ParsScanLayout(size_t P = 0, size_t S = 0, bool general = false, size_t chunk_ = 0) : chunk(chunk_)
  {
    Pp = (P + 1) & ~(size_t)1;
    plane_bytes = general ? S * Pp * sizeof(int) : Pp * 2 * sizeof(int);
    site_bytes = Pp * sizeof(int);
    site = keep + plane_bytes;
    recs = (site + site_bytes + 15) & ~(size_t)15;
    sums = recs + chunk * sizeof(ParsScanRec);
    tile_sums = sums + chunk * sizeof(unsigned long long);
    total = tile_sums + chunk * ((P + kRegraftTile - 1) / kRegraftTile) * sizeof(unsigned long long);
  }
};

// how a launch of n candidates over `tiles` pattern tiles is cut into slabs (the grid's second dimension): as many slabs as give
// every compute unit kParsScanSlabFactor workgroups, no more than candidates; every slab but the last holds `size` records
struct ParsScanSlabs
{
  size_t count = 0, size = 0;
  ParsScanSlabs(size_t n, size_t tiles, size_t compute_units, size_t factor = kParsScanSlabFactor)
  {
    if (n == 0) return;
    const size_t want = std::min(n, std::max<size_t>(1, (factor * compute_units + tiles - 1) / std::max<size_t>(1, tiles)));
    size = (n + want - 1) / want;
    count = (n + size - 1) / size;
  }
};

// a length's 64 bits -> its matrix slot, in first-seen order: identical lengths of a chunk are built once (+0.0 and -0.0, or two
// NaNs of different payloads, are different lengths here)
struct SlotTable
{
  std::vector<double>                         lengths; // [slot]
  std::unordered_map<unsigned long long, int> slot_of;
  void reset() { lengths.clear(), slot_of.clear(); }
  int slot(double l)
  {
    unsigned long long bits;
    memcpy(&bits, &l, sizeof bits);
    const auto it = slot_of.find(bits);
    if (it != slot_of.end()) return it->second;
    lengths.push_back(l);
    return slot_of[bits] = (int)lengths.size() - 1;
  }
};

inline RegraftRec regraft_pack(const phyhip_regraft_candidate &c, SlotTable &t)
{
  return RegraftRec{c.child1Partials, c.child2Partials, c.subtreePartials, c.flags, t.slot(c.child1Length), t.slot(c.child2Length),
                    t.slot(c.subtreeLength), 0};
}

} // namespace phyhip_host
#pragma GCC visibility pop
