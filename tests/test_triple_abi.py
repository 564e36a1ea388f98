"""Triple_Dist on the device through every layer that needs no GPU: both headers declare the new functions, the built libraries export
them, capi.SYMBOLS lists them, the bindings expose them, the two records are laid out as a C compiler lays them out (a compiled
sizeof / offsetof probe of include/phyhip.h against the ctypes mirrors), and the constants the bindings repeat are the kernel's.
CPU-only."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("phyhip_optimise_triples", "phyhip_get_triple_partials", "phyhip_set_triple_work_space", "phyhip_profile_read_triples")


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
    assert hasattr(lktree.load(), "Triple_Dist") and hasattr(lktree.load(), "Triple_Dist_Scan")


def test_the_abi_header_declares_them():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    want = {"phyhip_optimise_triples": ("int instance", "const phyhip_triple_candidate *candidates", "int count", "int iterMax", "double tol",
                                        "int keepCandidate", "phyhip_triple_result *outResults"),
            "phyhip_get_triple_partials": ("int instance", "int which", "double *outPartials", "int *outScaleFactors"),
            "phyhip_set_triple_work_space": ("int instance", "long long maxBytes"),
            "phyhip_profile_read_triples": ("int instance", "double *outKernelMs", "int *outCalls", "long long *outEvaluations")}
    for name, args in want.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, abi, flags=re.M)
        assert m, name
        got = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert got == list(args), (name, got)
    assert re.search(r"^#define PHYHIP_TRIPLE_NODE_IS_LEFT\(i\) \(1 << \(i\)\)", abi, flags=re.M)


def test_the_host_header_declares_triple_dist():
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^phydbl Triple_Dist\(t_node \*a, t_tree \*tree\);", lk, flags=re.M)
    assert re.search(r"^void Triple_Dist_Scan\(t_tree \*tree, int n, t_node \*\*a, phydbl \(\*l_out\)\[3\], phydbl \*lnL, int \*status\);", lk,
                     flags=re.M)


def test_the_ctypes_mirrors_match_the_c_structs(tmp_path):
    capi, lktree = _built()
    cand = [f[0] for f in capi.TripleCandidate._fields_]
    res = [f[0] for f in capi.TripleResult._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "phyhip.h"\nint main(void)\n{\n'
                   '  printf("%zu %zu\\n", sizeof(phyhip_triple_candidate), sizeof(phyhip_triple_result));\n' +
                   "".join('  printf("%%zu\\n", offsetof(phyhip_triple_candidate, %s));\n' % f for f in cand) +
                   "".join('  printf("%%zu\\n", offsetof(phyhip_triple_result, %s));\n' % f for f in res) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert nums[:2] == [C.sizeof(capi.TripleCandidate), C.sizeof(capi.TripleResult)] == [40, 96]
    k = 2
    for f in cand:
        assert getattr(capi.TripleCandidate, f).offset == nums[k], f
        k += 1
    for f in res:
        assert getattr(capi.TripleResult, f).offset == nums[k], f
        k += 1


def test_the_bindings_and_the_constants():
    capi, lktree = _built()
    for m in ("optimise_triples", "triple_partials", "set_triple_work_space", "profile_read_triples"):
        assert callable(getattr(capi.Instance, m, None)), m
    assert callable(getattr(lktree.LkTree, "Triple_Dist", None)) and callable(getattr(lktree.LkTree, "Triple_Dist_Scan", None))
    src = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_triple.hip")).read()
    assert int(re.search(r"constexpr long long kTripleMaxPatterns = (\d+);", src).group(1)) == capi.TRIPLE_MAX_PATTERNS
    assert int(re.search(r"constexpr int\s+kTripleIterMax = (\d+);", src).group(1)) == capi.BRENT_IT_MAX
    assert int(re.search(r"constexpr int\s+kTripleLkEnd = (\d+);", src).group(1)) == capi.TRIPLE_LK_END
    m = re.search(r"kTripleThreads = S == 4 \? (\d+) : (\d+);", src)
    assert {4: int(m.group(1)), 20: int(m.group(2))} == capi.TRIPLE_THREADS
    m = re.search(r"kTripleKeep = S == 4 \? (\d+) : (\d+);", src)
    assert {4: int(m.group(1)), 20: int(m.group(2))} == capi.TRIPLE_KEEP
    assert capi.triple_node_is_left(0) == 1 and capi.triple_node_is_left(2) == 4
    # ONE statement of the search's control flow, and of a probe: the kernel compiles the step header and calls dlk_lane
    assert "phyhip_brlen_step.h" in src and "brlen_step(&st" in src and "brlen_begin(&st" in src and "dlk_lane<S, CP>" in src
    assert "sqrt(" not in src
    # the joined vector, the product and the matrix body are the regraft scan's
    dev = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_regraft_dev.hpp")).read()
    scan = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_regraft.hip")).read()
    for fn in ("regraft_pmat_body", "regraft_join", "regraft_product"):
        assert ("void %s(" % fn in dev or "double %s(" % fn in dev) and fn + "<" in src and fn + "<" in scan, fn
        assert "void %s(" % fn not in scan and "double %s(" % fn not in scan, fn
    # the work-space arithmetic the bindings repeat
    assert capi.triple_chunk_candidates(382, 4, 4) > 64 and capi.triple_chunk_candidates(16384, 8, 20, 1) == 1


def test_the_translation_unit_is_in_the_build_list_with_the_search_kernels_flag():
    import __graft_entry__ as g
    units = dict(g.UNITS)
    assert units["phyhip_triple.hip"] == units["phyhip_brlen.hip"] == ["-mllvm", "-disable-machine-licm"]
