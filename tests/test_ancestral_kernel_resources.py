"""The kernel behind phyhip_calculate_node_state_posteriors (phyml_amd/csrc/phyhip_ancestral.hip) keeps its accumulators, the
running product and the side vector in registers -- 3 x 20 doubles per lane with 20 states: no scratch and no spills in either
instantiation, read -- as tests/test_kernel_resources.py does -- off the AMDGPU metadata notes of the BUILT product library.
CPU-only."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def posterior_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, "node_posterior_kernel", build=True)


def test_both_instantiations_are_there(posterior_kernels):
    assert len(posterior_kernels) == 2, sorted(posterior_kernels)
    assert any("node_posterior_kernelILi4E" in n for n in posterior_kernels)
    assert any("node_posterior_kernelILi20E" in n for n in posterior_kernels)


def test_no_scratch_and_no_spills(posterior_kernels):
    assert posterior_kernels
    for n, k in posterior_kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
