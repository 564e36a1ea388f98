"""The kernels of phyhip_calculate_regraft_log_likelihoods (phyml_amd/csrc/phyhip_regraft.hip): every instantiation of the scan kernel
-- <states, layout of the instance's buffers>: 4 states in host order and pattern-minor, 20 states in host order and fragment-major --
and of the matrix kernel is in the built library; none uses scratch or spills a vector or scalar register (the 4-state scan holds up
to 8 x 4 values per lane in registers until the scaling decision, the 20-state one computes them twice instead); none takes more than
16 KB of LDS (20 states: the three matrices of one category, 9.6 KB).  The only register budget asserted is what a resident 256-thread
workgroup implies: 512 unified registers per lane.  Read -- as tests/test_kernel_resources.py does -- off the AMDGPU metadata notes
of the BUILT product library; the counts are recorded in profiles/regraft_scan.md.  CPU-only."""
import pytest


@pytest.fixture(scope="module")
def regraft_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return {stem: kr.product_kernels(tmp_path_factory, stem, build=True) for stem in ("regraft_scan_kernel", "regraft_pmat_kernel", "regraft_sum_kernel")}


def test_every_instantiation_is_there_once(regraft_kernels):
    scan, pmat, total = regraft_kernels["regraft_scan_kernel"], regraft_kernels["regraft_pmat_kernel"], regraft_kernels["regraft_sum_kernel"]
    assert len(scan) == 4, sorted(scan)
    for ns, layout in ((4, 0), (4, 2), (20, 0), (20, 1)):
        assert sum(("regraft_scan_kernelILi%dELi%dEE" % (ns, layout)) in n for n in scan) == 1, (ns, layout, sorted(scan))
    assert len(pmat) == 2, sorted(pmat)
    for ns in (4, 20):
        assert sum(("regraft_pmat_kernelILi%dEE" % ns) in n for n in pmat) == 1, (ns, sorted(pmat))
    assert len(total) == 1, sorted(total)


def test_no_scratch_no_spills_lds_within_16_kb(regraft_kernels):
    for stem, kernels in regraft_kernels.items():
        assert kernels, stem
        for n, k in kernels.items():
            print(n, {f: k[f] for f in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")})
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
            assert k["group_segment_fixed_size"] <= 16 * 1024, (n, k)
            assert k["max_flat_workgroup_size"] == (64 if stem == "regraft_sum_kernel" else 256), (n, k)
            assert k["vgpr_count"] + k["agpr_count"] <= 512, (n, k)   # a 256-thread workgroup is resident; no tighter budget is claimed
