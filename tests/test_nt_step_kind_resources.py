"""The list-form nucleotide kernels with straight-line step bodies (phyml_amd/csrc/phyhip_nt2.hpp; profiles/r14_nt_step_kinds.md),
pinned on the code objects of the BUILT product library as tests/test_nt_record_resources.py does: no scratch, at most 256 vector
registers in the two-lane and mixed instantiations (two waves per SIMD), and in EVERY kernel that carries the bodies no more spilled
scalar registers than the same kernel had before them.  And what the host keeps per tip row: phyhip_tip_row_bits -- the count and
the predicate the setters of tip rows run (tip_row_counts, phyhip.hip) -- against a numpy restatement.  CPU-only."""
import re

import numpy as np
import pytest

from phyml_amd import capi
from test_kernel_resources import product_kernels

MIXED = "_ZN6phyhip25traverse_nt2_mixed_kernelILi4ELb{inl}EEEvNS_10TreeParamsEPKNS_8IssueRecEPKNS_7ExecRecEPKdPKhi"
LIST = re.compile(r"traverse_nt2_kernelILi(\d)ELi(\d)ELb0ELi0ELi2ELb([01])EEEv")   # <C, G, false, 0, 2, INL>

# sgpr_spill_count before the step bodies (profiles/r13_nt_records.md and the same build's code objects), of every kernel that
# carries them: nt2_bodied(C, G, INL) of phyhip_kernels.hpp -- (C, G, INL) -> count -- and the two mixed kernels
PARENT_SGPR_SPILLS = {(2, 2, 0): 16, (4, 2, 1): 8, (4, 4, 0): 16, "mixed0": 34, "mixed1": 34}
# ... and of the list forms that must not carry them (the bodies cost these two 12 -> 24 and 16 -> 26): the parent's figures, all
# of them -- with the vector registers, the sign that the generic step alone was compiled
PARENT_UNBODIED = {(4, 2, 0): (12, 191), (2, 2, 1): (16, 147), (1, 1, 0): (12, 125), (1, 1, 1): (20, 145), (2, 1, 0): (12, 191), (2, 1, 1): (16, 215),
                   (3, 1, 0): (16, 255), (3, 1, 1): (16, 298), (4, 1, 0): (24, 317), (4, 1, 1): (31, 374)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return product_kernels(tmp_path_factory, "traverse_nt2_kernel", "traverse_nt2_mixed_kernel", build=True)


def list_forms(kernels):
    out = {}
    for n in kernels:
        m = LIST.search(n)
        if m:
            out[tuple(int(g) for g in m.groups())] = kernels[n]
    out["mixed0"], out["mixed1"] = kernels[MIXED.format(inl=0)], kernels[MIXED.format(inl=1)]
    return out


def test_every_bodied_kernel_keeps_its_bounds(kernels):
    forms = list_forms(kernels)
    assert set(forms) == set(PARENT_SGPR_SPILLS) | set(PARENT_UNBODIED), sorted(map(str, forms))
    for key, parent in PARENT_SGPR_SPILLS.items():
        k = forms[key]
        print(key, {f: k[f] for f in ("vgpr_count", "sgpr_count", "sgpr_spill_count")})
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (key, k)
        if key != (4, 4, 0):
            assert k["vgpr_count"] <= 256, (key, k["vgpr_count"])        # two waves per SIMD
        else:
            assert k["vgpr_count"] <= 128, (key, k["vgpr_count"])        # four
        assert k["sgpr_spill_count"] <= parent, (key, k["sgpr_spill_count"], parent)


def test_the_other_list_forms_are_the_parents(kernels):
    forms = list_forms(kernels)
    for key, (spills, vgprs) in PARENT_UNBODIED.items():
        k = forms[key]
        assert (k["sgpr_spill_count"], k["vgpr_count"]) == (spills, vgprs), (key, k["sgpr_spill_count"], k["vgpr_count"])
        assert k["private_segment_fixed_size"] == 0


def numpy_bits(codes):
    codes = np.asarray(codes, dtype=np.uint8)
    return int(np.isin(codes, (1, 2, 4, 8)).all()) | (int((codes == 15).any()) << 1)


def test_row_bits_against_numpy():
    rng = np.random.default_rng(14)
    seen = set()
    for n in (1, 3, 63, 64, 65, 96, 8230):
        onehot = (1 << rng.integers(0, 4, n)).astype(np.uint8)
        rows = [onehot, np.full(n, 15, np.uint8), rng.integers(1, 16, n).astype(np.uint8), np.zeros(n, np.uint8)]
        last = onehot.copy(); last[-1] = 5      # the one ambiguous code is the row's last pattern, inside the padded wave
        last15 = onehot.copy(); last15[-1] = 15
        first = onehot.copy(); first[0] = 14
        for row in rows + [last, last15, first]:
            got = capi.tip_row_bits(row)
            assert got == numpy_bits(row), (n, row[:8], got)
            seen.add(got)
    assert capi.tip_row_bits(np.full(96, 15, np.uint8)) == 2 and capi.tip_row_bits(np.array([1, 2, 4, 8], np.uint8)) == 1
    assert seen == {0, 1, 2}    # (one-hot throughout and a 15 exclude each other)
