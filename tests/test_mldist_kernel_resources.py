"""The kernels behind phyhip_calculate_pairwise_ml_distances (phyml_amd/csrc/phyhip_dist.hip) keep what they hold in registers and
LDS -- the count kernel its four accumulator blocks, the optimiser the state of Dist_F_Brent (its matrices live in LDS): no
scratch and no spills in any instantiation, read -- as tests/test_kernel_resources.py does -- off the AMDGPU metadata notes of the
BUILT product library.  CPU-only."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dist_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, "dist_count_kernel", "dist_sums_kernel", "dist_opt_kernel", "dist_add_kernel", build=True)


def test_every_instantiation_is_there(dist_kernels):
    assert len(dist_kernels) == 7, sorted(dist_kernels)
    for stem in ("dist_count_kernel", "dist_sums_kernel", "dist_opt_kernel"):
        for s in (4, 20):
            assert any("%sILi%dE" % (stem, s) in n for n in dist_kernels), (stem, s)


def test_no_scratch_and_no_spills(dist_kernels):
    assert dist_kernels
    for n, k in dist_kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
