"""The search kernel of phyhip_optimise_edge_length (phyml_amd/csrc/phyhip_brlen.hip) is ONE workgroup whose waves must all be
resident and which keeps a lane's first rounds of products in registers across the probes: every <S, CP> instantiation is there, none
uses scratch or spills, and each stays within 512 / (workgroup threads / 256) unified registers -- 128 for the 1024 threads at 4
states, 256 for the 512 threads at 20 states (dlk_lane's working set at 20 states is about 160 registers by itself).  Read -- as
tests/test_kernel_resources.py does -- off the AMDGPU metadata notes of the BUILT product library.  CPU-only."""
import pytest

STEM = "brlen_opt_kernel"


@pytest.fixture(scope="module")
def brlen_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, STEM, build=True)


def test_every_shape_is_there_once(brlen_kernels):
    assert len(brlen_kernels) == 8, sorted(brlen_kernels)
    for ns in (4, 20):
        for cp in (1, 2, 4, 8):
            assert sum(("ILi%dELi%dEE" % (ns, cp)) in n for n in brlen_kernels) == 1, (ns, cp, sorted(brlen_kernels))


def test_no_scratch_no_spills_and_all_waves_resident(brlen_kernels):
    from phyml_amd import capi
    assert brlen_kernels
    for n, k in brlen_kernels.items():
        ns = 4 if "ILi4ELi" in n else 20
        threads = capi.BRLEN_THREADS[ns]
        assert k["max_flat_workgroup_size"] == threads, (n, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] + k["agpr_count"] <= 512 // (threads // 256), (n, k)
        assert k["group_segment_fixed_size"] <= 4096, (n, k)   # the expl table, the waves' sums and the search state
