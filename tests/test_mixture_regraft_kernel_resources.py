"""The kernels of phyhip_calculate_mixture_regraft_log_likelihoods (phyml_amd/csrc/phyhip_regraft.hip): every instantiation of the scan
kernel over the classes -- <states, layout of the class instances' buffers>: 4 states in host order and pattern-minor, 20 states in
host order and fragment-major -- and of the matrix kernel is in the built library once; none uses scratch or spills a vector or scalar
register (a class has one category: its joined vector is S values held in registers at both state counts, one pass); none takes more
than 16 KB of LDS (20 states: the three matrices of one class, 9.6 KB); a resident 256-thread workgroup implies at most 512 unified
registers per lane.  Read -- as tests/test_regraft_kernel_resources.py does -- off the AMDGPU metadata notes of the BUILT product
library; the counts are recorded in profiles/mixture_regraft_scan.md.  CPU-only."""
import pytest

STEMS = ("mixregraft_classes_kernel", "mixregraft_matrices_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return {stem: kr.product_kernels(tmp_path_factory, stem, build=True) for stem in STEMS}


def test_every_instantiation_is_there_once(kernels):
    scan, pmat = kernels["mixregraft_classes_kernel"], kernels["mixregraft_matrices_kernel"]
    assert len(scan) == 4, sorted(scan)
    for ns, layout in ((4, 0), (4, 2), (20, 0), (20, 1)):
        assert sum(("mixregraft_classes_kernelILi%dELi%dEE" % (ns, layout)) in n for n in scan) == 1, (ns, layout, sorted(scan))
    assert len(pmat) == 2, sorted(pmat)
    for ns in (4, 20):
        assert sum(("mixregraft_matrices_kernelILi%dEE" % ns) in n for n in pmat) == 1, (ns, sorted(pmat))
    # the names stay clear of the plain scan's, which tests/test_regraft_kernel_resources.py selects by substring and counts
    for n in list(scan) + list(pmat):
        assert not any(s in n for s in ("regraft_scan_kernel", "regraft_pmat_kernel", "regraft_sum_kernel")), n


def test_no_scratch_no_spills_lds_within_16_kb(kernels):
    for stem, ks in kernels.items():
        assert ks, stem
        for n, k in ks.items():
            print(n, {f: k[f] for f in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")})
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
            assert k["group_segment_fixed_size"] <= 16 * 1024, (n, k)
            assert k["max_flat_workgroup_size"] == 256, (n, k)
            assert k["vgpr_count"] + k["agpr_count"] <= 512, (n, k)
