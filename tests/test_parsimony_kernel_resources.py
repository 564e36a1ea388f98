"""The parsimony kernels (phyml_amd/csrc/phyhip_pars.hip) keep what they hold in registers: no scratch and no spills, read -- as
tests/test_kernel_resources.py does -- off the AMDGPU metadata notes of the BUILT product library.  Both kernels are there once per
state count (4 and 20).  Planned register budgets: the Fitch kernel holds two children, the result and the two prefetched children of
the next operation, two patterns each (five int4) plus addresses -- at most 64 VGPRs, eight waves per SIMD, since only other waves hide
its loads; the step-matrix kernel holds both children's states (2 x 20 ints at 20 states), the matrix in LDS -- at most 96 VGPRs, five
waves per SIMD.  CPU-only."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ("pars_fitch_kernel", "pars_general_kernel")


@pytest.fixture(scope="module")
def pars_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, *STEMS, build=True)


def test_both_kernels_are_there_once_per_state_count(pars_kernels):
    assert len(pars_kernels) == 4, sorted(pars_kernels)
    for stem in STEMS:
        for ns in (4, 20):
            assert sum(stem in n and ("ILi%dE" % ns) in n for n in pars_kernels) == 1, (stem, ns, sorted(pars_kernels))


def test_no_scratch_no_spills_and_the_planned_registers(pars_kernels):
    assert pars_kernels
    for n, k in pars_kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] <= (64 if "pars_fitch_kernel" in n else 96), (n, k)
    for n, k in pars_kernels.items():   # the step matrix is the only LDS: S * S ints
        if "pars_general_kernel" in n:
            assert k["group_segment_fixed_size"] == (1600 if "ILi20E" in n else 64), (n, k)
        else:
            assert k["group_segment_fixed_size"] == 0, (n, k)
