"""The regraft scan through every layer that needs no GPU: both headers declare the new functions, the built libraries export them,
capi.SYMBOLS lists them, the bindings expose them, phyhip_regraft_candidate is 40 bytes with the header's field offsets (a compiled
sizeof / offsetof probe of include/phyhip.h against the ctypes mirror), and the constants the bindings repeat are the unit's.
CPU-only."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"phyhip_calculate_regraft_log_likelihoods": ("int instance", "int eigenIndex", "const phyhip_regraft_candidate *candidates", "int count",
                                                      "int keepCandidate", "double *outLogLikelihoods", "int *outWarnings"),
         "phyhip_get_regraft_partials": ("int instance", "double *outPartials", "int *outScaleFactors"),
         "phyhip_get_regraft_transition_matrix": ("int instance", "int candidate", "int which", "double *outMatrix"),
         "phyhip_set_regraft_work_space": ("int instance", "long long maxBytes"),
         "phyhip_profile_read_regraft": ("int instance", "double *outKernelMs", "int *outCalls", "long long *outCandidates")}
FIELDS = ("child1Partials", "child2Partials", "subtreePartials", "flags", "child1Length", "child2Length", "subtreeLength")


def _built():
    import __graft_entry__ as g
    g.build()
    from phyml_amd import capi, lktree
    return capi, lktree


def test_the_library_exports_the_entry_points():
    capi, lktree = _built()
    L = capi.load()
    for name in ENTRY:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name
    assert hasattr(lktree.load(), "Lk_Regraft_Scan")


def test_the_abi_header_declares_them():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    for name, args in ENTRY.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, abi, flags=re.M)
        assert m, name
        got = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert got == list(args), (name, got)
    assert re.search(r"^#define PHYHIP_REGRAFT_SUBTREE_IS_LEFT 1\b", abi, flags=re.M)
    # the header says what happens above 8 categories
    assert "MORE THAN 8" in abi and "refused, not served" in abi


def test_the_host_header_declares_the_scan():
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^void Lk_Regraft_Scan\(t_tree \*tree, t_edge \*b_sub, t_node \*d_sub, int link_is_left, phydbl l_sub,\s*"
                     r"int n, t_edge \*const \*b_target, const phydbl \*l_left, const phydbl \*l_rght, phydbl \*lnL\);", lk, flags=re.M)
    assert "INTACT tree" in lk   # what the vectors are without Prune_Subtree / Graft_Subtree


def test_the_candidate_struct_is_40_bytes_with_the_headers_offsets(tmp_path):
    capi, _ = _built()
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "phyhip.h"\nint main(void)\n{\n'
                   '  printf("%zu\\n", sizeof(phyhip_regraft_candidate));\n' +
                   "".join('  printf("%%zu\\n", offsetof(phyhip_regraft_candidate, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert nums[0] == 40 == C.sizeof(capi.RegraftCandidate)
    assert nums[1:] == [0, 4, 8, 12, 16, 24, 32]
    assert [f[0] for f in capi.RegraftCandidate._fields_] == list(FIELDS)
    assert [getattr(capi.RegraftCandidate, f).offset for f in FIELDS] == nums[1:]


def test_the_bindings_and_the_constants():
    capi, lktree = _built()
    for m in ("regraft_log_likelihoods", "regraft_partials", "regraft_transition_matrix", "set_regraft_work_space", "profile_read_regraft"):
        assert callable(getattr(capi.Instance, m, None)), m
    assert callable(getattr(lktree.LkTree, "Regraft_Scan", None))
    src = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_regraft.hip")).read()
    side = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_side.hpp")).read()
    plan = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_scan_plan.hpp")).read()
    driver = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_scan.hpp")).read()
    assert int(re.search(r"constexpr int\s+kRegraftTile = (\d+);", plan).group(1)) == capi.REGRAFT_TILE
    assert int(re.search(r"constexpr int kRegraftMaxCategories = (\d+);", src).group(1)) == capi.REGRAFT_MAX_CATEGORIES
    assert "kRegraftWorkBytes = kDistBandBytes" in side and "kDistBandBytes = 128u << 20" in side and capi.REGRAFT_WORK_BYTES == 128 << 20
    assert capi.REGRAFT_SUBTREE_IS_LEFT == 1
    # the work-space arithmetic of the header, as the bindings restate it: the default bound holds every candidate of a whole scan of
    # the small examples in one chunk, and a bound of a few candidates cuts a list of 37 into at least three
    assert capi.regraft_chunk_candidates(382, 4, 4) >= 512 and capi.regraft_chunk_candidates(429, 4, 20) >= 512
    fixed = 300 * 4 * 4 * 8 + 300 * 4
    per = 3 * 4 * 4 * 4 * 8 + 2 * 8 + 72
    assert capi.regraft_chunk_candidates(300, 4, 4, fixed + 12 * per) == 12
    assert capi.regraft_chunk_candidates(300, 4, 4, 1) == 1
    # no floating-point atomics, no cooperative launch, no new environment switch in the unit
    for word in ("atomicAdd", "hipLaunchCooperativeKernel", "getenv(", "diag_env("):
        assert word not in src and word not in plan and word not in driver, word


def test_the_translation_unit_is_in_the_build_list():
    import __graft_entry__ as g
    assert "phyhip_regraft.hip" in dict(g.UNITS)
