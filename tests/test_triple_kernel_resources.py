"""The kernel of phyhip_optimise_triples (phyml_amd/csrc/phyhip_triple.hip) runs one workgroup per candidate whose waves must all be
resident: every <S, CP, L> instantiation is there -- both state counts, four category paddings, host order and the state count's own
buffer layout -- none reserves scratch or spills a vector register.  The kernel's many uniform values -- the pointers and constants of
four phases -- do not all fit the 102 scalar registers: the compiler parks some in lanes of vector registers, inside the register
budget, which costs no memory traffic (private_segment_fixed_size == 0 says none of it reaches memory).  That is allowed up to the
192 lanes of three vector registers, not without bound (70-126 at the time of writing, instantiation by instantiation).  Each stays within
512 / (workgroup threads / 256) unified registers (256 for the 512 threads at 4 states, 512 for the 256 threads at 20 states), and
its LDS -- the expl table, the staged matrices (all categories at 4 states, one at 20), the
eigenvectors, the matrix builder's scratch, the search state and the result record -- stays below 32 KiB, so that two workgroups fit a
compute unit's 64 KiB window whatever the allocation granularity.  Read -- as tests/test_kernel_resources.py does -- off the AMDGPU
metadata notes of the BUILT product library.  CPU-only."""
import pytest

STEM = "triple_kernel"


@pytest.fixture(scope="module")
def triple_kernels(tmp_path_factory):
    import test_kernel_resources as kr
    return kr.product_kernels(tmp_path_factory, STEM, build=True)


def test_every_shape_is_there_once(triple_kernels):
    assert len(triple_kernels) == 16, sorted(triple_kernels)
    for ns, layouts in ((4, (0, 2)), (20, (0, 1))):
        for cp in (1, 2, 4, 8):
            for lay in layouts:
                assert sum(("ILi%dELi%dELi%dEE" % (ns, cp, lay)) in n for n in triple_kernels) == 1, (ns, cp, lay, sorted(triple_kernels))


def test_no_scratch_no_vector_spills_and_all_waves_resident(triple_kernels):
    from phyml_amd import capi
    assert triple_kernels
    for n, k in triple_kernels.items():
        ns = 4 if "ILi4ELi" in n else 20
        threads = capi.TRIPLE_THREADS[ns]
        assert k["max_flat_workgroup_size"] == threads, (n, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
        assert k["sgpr_spill_count"] <= 3 * 64, (n, k)
        # (.vgpr_count of a gfx950 code object is the unified file's: the accumulation registers -- at 20 states the lane-per-pattern
        # passes park values there instead of in memory -- are part of it: 256 + agpr_count where any are used)
        assert k["vgpr_count"] <= 512 // (threads // 256) and k["agpr_count"] <= max(0, k["vgpr_count"] - 256), (n, k)
        assert k["group_segment_fixed_size"] <= 32768, (n, k)
