"""The kernels behind phyhip_calculate_sh_support (phyml_amd/csrc/phyhip_support.hip) keep what they hold in registers -- the draw
kernel its three partial sums, the Philox block and the rows in flight: no scratch and no spills, read -- as
tests/test_kernel_resources.py does -- off the AMDGPU metadata notes of the BUILT product library.  States play no part in them: one
instantiation each.  CPU-only."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ("support_table_kernel", "support_totals_kernel", "support_draw_kernel", "support_count_kernel")


@pytest.fixture(scope="module")
def support_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, *STEMS, build=True)


def test_every_kernel_is_there_once(support_kernels):
    assert len(support_kernels) == 4, sorted(support_kernels)
    for stem in STEMS:
        assert sum(stem in n for n in support_kernels) == 1, stem


def test_no_scratch_and_no_spills(support_kernels):
    assert support_kernels
    for n, k in support_kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
    draw = [k for n, k in support_kernels.items() if "support_draw_kernel" in n][0]
    assert draw["vgpr_count"] <= 64, draw   # eight waves per SIMD: the gather hides its latency behind other replicates
