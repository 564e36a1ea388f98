"""The kernels of the parsimony regraft scan (phyml_amd/csrc/phyhip_pars.hip: pars_regraft_fitch, pars_regraft_general) keep what
they hold in registers: no scratch and no spills -- conditions, not measurements -- read, as tests/test_kernel_resources.py does, off
the AMDGPU metadata notes of the BUILT product library.  Each kernel is there once per state count (4 and 20).

LDS, exactly what the code declares (capi.PARS_REGRAFT_LDS): the cross-wave sum keeps two sets of one 8-byte slot per wave, so that
one barrier per candidate is enough -- 2 x 2 x 8 = 32 bytes in the Fitch kernel (128 lanes), 2 x 4 x 8 = 64 in the step-matrix
kernel (256 lanes), which adds its S * S ints of matrix.

Register plans:
  * Fitch: three operands (child 1, child 2, subtree), the two (at a subtree change three) prefetched operands of the next record and
    the join, two patterns each -- seven int4 = 28 registers --, the two 64-bit weights, the pattern's address parts and the
    reduction: at most 64 VGPRs, eight waves per SIMD, as the Fitch kernel of the operation lists.
  * step matrix: S minima of the subtree + 2 S operands + S results.  At 4 states everything is unrolled: 4 x 4 values, the 16 matrix
    entries the compiler keeps in registers, one candidate's 3 x 16 sums in flight at most, the weight and addresses: at most 80
    VGPRs, six waves per SIMD.  At 20 states the loops over the parent state stay loops (unrolled, the 400 matrix entries are
    hoisted and spill), so the S results and the S minima are registers chosen by the loop index: each such array is a register
    tuple of the next power of two, 32; the two operand arrays land in such tuples too (4 x 32 = 128), one row's 2 x 20 sums and 8
    matrix entries are in flight (48), the weight, addresses and the reduction take the rest: at most 208 VGPRs, two waves per SIMD.
    The kernel is bound by its 1 200 add-and-minimum pairs per candidate and pattern, not by the latency other waves would hide.
CPU-only."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ("pars_regraft_fitch", "pars_regraft_general")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, *STEMS, build=True)


def test_each_kernel_is_there_once_per_state_count(kernels):
    assert len(kernels) == 4, sorted(kernels)
    for stem in STEMS:
        for ns in (4, 20):
            assert sum(stem in n and ("ILi%dE" % ns) in n for n in kernels) == 1, (stem, ns, sorted(kernels))
    # ... and none of them is counted among the kernels of the operation lists (tests/test_parsimony_kernel_resources.py)
    assert not any("pars_fitch_kernel" in n or "pars_general_kernel" in n for n in kernels)


def test_no_scratch_no_spills_the_declared_lds_and_the_planned_registers(kernels):
    from phyml_amd import capi
    assert kernels
    for n, k in kernels.items():
        ns = 20 if "ILi20E" in n else 4
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        if "pars_regraft_fitch" in n:
            assert k["group_segment_fixed_size"] == capi.PARS_REGRAFT_LDS["fitch"] == 32, (n, k)
            assert k["vgpr_count"] <= 64, (n, k)
        else:
            assert k["group_segment_fixed_size"] == ns * ns * 4 + capi.PARS_REGRAFT_LDS["general"] == ns * ns * 4 + 64, (n, k)
            assert k["vgpr_count"] <= (208 if ns == 20 else 80), (n, k)
