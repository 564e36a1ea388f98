// phyhip_tail.hpp -- the per-pattern end of Lk_Core (src/lk.c:820-856 with Invariant_Lk, :1226-1273): ONE definition of the
// arithmetic the evaluation kernels end with, with what they intend to do differently as named parameters (DESIGN §5 says which
// kernel takes which, and which kernels still carry a copy of the tail's text around their call of invariant_lk).  Device
// functions only, no kernels, no host type; included from phyhip_kernels.hpp behind the constants, dev_exp and raise_warn, which it
// uses, and through it by every unit.  Results leave through reference parameters, not return values: inlined that way the
// callers compile to the machine code they had when each carried its own copy (profiles/r10_tail_refactor.md).
#pragma once

namespace phyhip
{

// Invariant_Lk's value for a pattern with a constant state (src/lk.c:1244-1258): inv = pi[that state] brought to the scale 2^f of
// the site likelihood, in pieces of at most 2^63 as the reference multiplies them (each exact, or the overflow to inf that `issue`
// reports).  f is a sum of scale exponents: every one of them starts at 0 (tips have none) and only ever grows by kLarge (the
// 2^256 rule of the partial updates, src/avx.c:504-510: sum = s1 + s2 [+ 256], here as in the CPU restatement), and the
// tails store either that sum or 0 as fact_sum_scale -- so f >= 0 always, and f == 0 multiplies once by 2^0: the reference's
// do-while needs no guard.
__device__ __forceinline__ void invariant_lk(double &inv, bool &issue, const double pi_iv, const int f, const int apply_scaling)
{
  inv = pi_iv;
  if (apply_scaling)
  {
    int e = f;
    do
    {
      const int piece = e < 63 ? e : 63;
      inv *= (double)(1ull << piece);
      e -= piece;
    } while (e != 0);
  }
  issue = isinf(inv);
}

// The +I mix of src/lk.c:820-842.  The reference's binary contracts site * (1 - pinvar) + inv * pinvar into one fused operation
// (one rounding).  The launched evaluation kernels round twice (the plain expression under -ffp-contract=off): their per-site
// outputs are held to 1e-12 / 1e-10, not to the bit, and tests/test_gpu_eigen_terms.py::test_tail_branches_on_the_hot_path
// pins their doubles as they are.  The exact route and dlk_lane are held to the reference's bits (tests/test_gpu_exact_site.py,
// tests/test_gpu_eigen_terms.py::test_per_pattern_terms*) and fuse.
enum class TailMix { two_roundings, fused };
// log / exp of the tail: the device library's log with dev_exp and a separately rounded LOG2 * f, or the reference's libm
// (phyhip_log.hpp, phyhip_exp.hpp) with fma(-f, LOG2, log) as the reference's binary has it -- the exact route, whose outputs are
// all present and whose warning flag is a buffer of its own that nobody polls (a plain store; no null tests, no fence).
enum class TailLibm { device, reference };
// Where the pattern's invariant state and pi[that state] come from: memory, read where the reference reads them, or what the
// caller fetched ahead (iv_pre, inv_pre: the argument form of the 20-state kernel holds both in registers).
enum class TailInputs { memory, preloaded };

template <TailMix MIX> __device__ __forceinline__ double mix_invariant(const double site, const double inv, const double pinvar)
{
  if constexpr (MIX == TailMix::fused) return __builtin_fma(site, 1. - pinvar, inv * pinvar);
  else return site * (1. - pinvar) + inv * pinvar;
}

// The SMALL floor with its warning (src/lk.c:847-851), then lsl = log(site) - LOG2 * f (:854).  `site` comes back floored.
template <TailLibm LIBM> __device__ __forceinline__ void floored_log(double &lsl, double &site, const int f, int *warn)
{
  if (site < kSmall)
  {
    site = kSmall;
    if constexpr (LIBM == TailLibm::reference) *warn = 1;
    else raise_warn(warn);
  }
  if constexpr (LIBM == TailLibm::reference) lsl = __builtin_fma(-(double)f, kLog2, phyhip_log_ref(site, phyhip_log_data));
  else lsl = log(site) - kLog2 * (double)f;
}

struct PlainStore
{
  template <class T> __device__ __forceinline__ void operator()(T *ptr, const T v) const { *ptr = v; }
};

// One pattern's tail: w the pattern's weight, `site` the category mixture (src/lk.c:816-818), f the sum of the two sides' scale
// exponents (0 without scaling).  Stores c_lnL_sorted, cur_site_lk and fact_sum_scale (with the overflow branch's reset to 0)
// through `st`, and sets contrib to the pattern's term w * lsl (src/lk.c:856; untouched for a pattern without weight, whose
// fact_sum_scale is still stored).  Q: TreeParams or the exact route's parameters.
template <TailMix MIX, TailLibm LIBM, TailInputs IN = TailInputs::memory, class Q, class Store>
__device__ __forceinline__ void site_tail(double &contrib, const Q &q, const size_t p, const double w, double site, int f, const Store &st,
                                          const int iv_pre = -1, const double inv_pre = 0.0)
{
  constexpr bool kAllOutputs = LIBM == TailLibm::reference;
  if (w > kSmall)
  {
    if (q.invar_model)
    {
      const int iv = IN == TailInputs::memory ? (int)q.invar[p] : iv_pre;
      double    inv = 0.0;
      bool      issue = false;
      if (iv >= 0) invariant_lk(inv, issue, IN == TailInputs::preloaded ? inv_pre : q.pi[iv], f, q.apply_scaling);
      if (issue)
      {
        f    = 0;
        site = q.pi[iv] * q.pinvar;
      }
      else
        site = mix_invariant<MIX>(site, inv, q.pinvar);
    }
    double lsl;
    floored_log<LIBM>(lsl, site, f, q.warn);
    if (kAllOutputs || q.site_lnl) st(&q.site_lnl[p], lsl);
    if constexpr (LIBM == TailLibm::reference) st(&q.site_lk[p], phyhip_exp_ref(lsl, phyhip_exp_tab));
    else if (q.site_lk) st(&q.site_lk[p], dev_exp(lsl));
    contrib = w * lsl;
  }
  st(&q.fact[p], f);
}

} // namespace phyhip
