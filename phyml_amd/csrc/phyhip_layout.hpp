// phyhip_layout.hpp -- where one entry of a partials buffer and one tip's state set lie in device memory, for the kernels beside
// the hot path that read whatever layout the instance holds (phyhip_exact.hip, phyhip_ancestral.hip).
// Internal: nothing here is part of the ABI (include/phyhip.h).
#pragma once
#include "phyhip_host.hpp"

namespace phyhip_host
{

// layout of an instance's internal buffers as such a kernel is told it: 0 host order [pattern][category][state], 1 fragment-major
// 20-state (aa_off, phyhip_aa.hpp), 2 pattern-minor 4-state pairs (phyhip_nt2.hpp)
inline int layout_of(const Instance *I) { return I->perm ? 1 : (I->soa ? 2 : 0); }

// element offset of (pattern, category, state) inside internal buffer b (dev_off of phyhip_host.hpp, for the device)
template <int S>
__device__ __forceinline__ size_t partial_off(int layout, long long P, long long Ppad, int C, int b, long long p, int c, int s)
{
  if (S == 20 && layout == 1) return (size_t)b * aa_buf_elems(Ppad, C) + aa_off(p, C, c, s);
  if (S == 4 && layout == 2)
    return (size_t)b * ((size_t)Ppad * C * S) + ((size_t)(c * 2 + (s >> 1)) * Ppad + (size_t)p) * 2 + (size_t)(s & 1);
  return (((size_t)b * P + (size_t)p) * C + c) * S + s;
}

// the allowed-state mask of tip `tip` at pattern p (tip t at t * Ppad; 4 states: the byte is the state set; 20: an index into code_masks)
template <int S>
__device__ __forceinline__ uint32_t tip_state_mask(const uint8_t *tip_codes, const uint32_t *code_masks, long long Ppad, int tip, long long p)
{
  const uint32_t code = tip_codes[(size_t)tip * Ppad + p];
  return (S <= 8) ? code : code_masks[code];
}

} // namespace phyhip_host
