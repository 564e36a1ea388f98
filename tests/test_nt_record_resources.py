"""The list-form nucleotide kernels after the move to compact step records (phyml_amd/csrc/phyhip_kernels.hpp: NtIssue / NtExec;
profiles/r13_nt_records.md), pinned on the code objects of the BUILT product library as tests/test_kernel_resources.py does: no
scratch, the waves per SIMD their launch bounds ask for, and fewer scalar registers spilled in the benchmark's kernel than the
descriptor records cost it.  CPU-only."""
import re

import pytest

from test_kernel_resources import product_kernels, waves_per_simd

# sgpr_spill_count of traverse_nt2_mixed_kernel<4, true> with descriptor records (a step kept two 24-word issue records and two
# 8-word execute records live): the figure the request for compact records was made on, profiles/r13_nt_records.md
PARENT_SGPR_SPILLS = 48

MIXED = "_ZN6phyhip25traverse_nt2_mixed_kernelILi4ELb{inl}EEEvNS_10TreeParamsEPKNS_8IssueRecEPKNS_7ExecRecEPKdPKhi"
# <C, G, DBG = false, ARGS = 0 (list form), DIST = 2, INL>: every list form the product launches (DIST = 1 is a diag-build switch)
LIST = re.compile(r"traverse_nt2_kernelILi(\d)ELi(\d)ELb0ELi0ELi2ELb([01])EEEv")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return product_kernels(tmp_path_factory, "traverse_nt2_kernel", "traverse_nt2_mixed_kernel", build=True)


def list_forms(kernels):
    """{name: waves per SIMD asked for} of the list-form kernels"""
    out = {n: int(LIST.search(n).group(2)) for n in kernels if LIST.search(n)}
    for inl in (0, 1):
        out[MIXED.format(inl=inl)] = 2
    return out


def test_the_list_forms_are_all_there(kernels):
    forms = list_forms(kernels)
    # (C, G) of launch_soa x with / without in-step children (G = 4: without only), and the two mixed kernels
    assert len(forms) == 6 * 2 + 1 + 2, sorted(forms)
    for n in forms:
        assert n in kernels, n


def test_list_form_kernels_have_no_scratch(kernels):
    for n in list_forms(kernels):
        k = kernels[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)


def test_list_form_kernels_keep_their_waves_per_simd(kernels):
    for n, g in list_forms(kernels).items():
        assert waves_per_simd(kernels[n]["vgpr_count"]) >= g, (n, kernels[n]["vgpr_count"], g)


def test_the_benchmarks_kernel_spills_fewer_scalar_registers(kernels):
    k = kernels[MIXED.format(inl=1)]
    print("traverse_nt2_mixed_kernel<4, true>:", {f: k[f] for f in ("sgpr_count", "sgpr_spill_count", "vgpr_count")})
    assert k["sgpr_spill_count"] < PARENT_SGPR_SPILLS, k
