"""The kernel behind phyhip_calculate_edge_site_outputs_exact (phyml_amd/csrc/phyhip_exact.hip) keeps its 20 accumulators and 20
left-side values in registers: no scratch and no spills in either instantiation, read -- as tests/test_kernel_resources.py does --
off the AMDGPU metadata notes of the BUILT product library.  CPU-only."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exact_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, "exact_site", build=True)


def test_both_instantiations_are_there(exact_kernels):
    assert len(exact_kernels) == 2, sorted(exact_kernels)
    assert any("exact_site_kernelILi4E" in n for n in exact_kernels) and any("exact_site_kernelILi20E" in n for n in exact_kernels)


def test_no_scratch_and_no_spills(exact_kernels):
    assert exact_kernels
    for n, k in exact_kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
