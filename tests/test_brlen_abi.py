"""Br_Len_Opt on the device through every layer that needs no GPU: both headers declare the new functions, the built libraries export
them, capi.SYMBOLS lists them, the bindings expose them, the appended struct fields sit where a C compiler puts them (a compiled
sizeof / offsetof probe of include/phyhip_lk.h against the ctypes mirrors), and the constants the bindings repeat are the kernel's.
CPU-only."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("phyhip_optimise_edge_length", "phyhip_profile_read_edge_length")


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
    assert hasattr(lktree.load(), "Br_Len_Opt") and hasattr(lktree.load(), "Br_Len_Newton")


def test_the_abi_header_declares_them():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    want = {"phyhip_optimise_edge_length": ("int instance", "double *l", "double initLnL", "int iterMax", "double tol", "double *outLnL",
                                            "double *outDLnL", "int *outEvaluations", "int *outStatus"),
            "phyhip_profile_read_edge_length": ("int instance", "double *outKernelMs", "int *outCalls", "long long *outEvaluations")}
    for name, args in want.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, abi, flags=re.M)
        assert m, name
        got = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert got == list(args), (name, got)


def test_the_host_header_declares_br_len_opt_and_appends_the_fields():
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^phydbl Br_Len_Opt\(phydbl \*l, t_edge \*b, t_tree \*tree\);", lk, flags=re.M)
    assert re.search(r"^phydbl Br_Len_Newton\(phydbl \*l, t_edge \*b, t_tree \*tree\);", lk, flags=re.M)   # stays
    assert re.search(r"^#define BRENT_IT_MAX 1000\b", lk, flags=re.M)
    body = lk[lk.index("typedef struct __Tree"):lk.index("} t_tree;")]
    order = [body.index(f) for f in ("sh_seed;", "own_step_mat;", "n_tot_bl_opt;", "bl_opt_evaluations, bl_opt_status;", "bl_opt_host_chain;")]
    assert order == sorted(order)   # after everything that was there
    body = lk[lk.index("typedef struct __Model"):lk.index("} t_mod;")]
    order = [body.index(f) for f in ("use_m4mod;", "min_diff_lk_local;", "brent_it_max;")]
    assert order == sorted(order)


def test_the_ctypes_mirrors_match_the_c_structs(tmp_path):
    capi, lktree = _built()
    src = tmp_path / "probe.c"
    fields_tree = [f[0] for f in lktree.t_tree_brlen._fields_ if f[0] != "alias_one_subpatt"]
    fields_mod = [f[0] for f in lktree.t_mod_brlen._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "phyhip_lk.h"\nint main(void)\n{\n'
                   '  printf("%zu %zu %zu\\n", sizeof(t_tree), sizeof(t_mod), sizeof(t_edge));\n' +
                   "".join('  printf("%%zu\\n", offsetof(t_tree, %s));\n' % f for f in fields_tree) +
                   "".join('  printf("%%zu\\n", offsetof(t_mod, %s));\n' % f for f in fields_mod) +
                   '  printf("%zu %zu\\n", offsetof(t_tree, own_step_mat), offsetof(t_mod, use_m4mod));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    nums = [int(x) for x in out]
    assert nums[:3] == [C.sizeof(lktree.t_tree_brlen), C.sizeof(lktree.t_mod_brlen), C.sizeof(lktree.t_edge)]
    k = 3
    for f in fields_tree:
        assert getattr(lktree.t_tree_brlen, f).offset == nums[k], f
        k += 1
    for f in fields_mod:
        assert getattr(lktree.t_mod_brlen, f).offset == nums[k], f
        k += 1
    assert nums[k] == lktree.t_tree_pars.own_step_mat.offset and nums[k + 1] == lktree.t_mod.use_m4mod.offset   # nothing earlier moved
    assert issubclass(lktree.t_mod_brlen, lktree.t_mod)
    n_old = len(lktree.t_tree._fields_) + len(lktree.t_tree_pars._fields_)
    assert [f[0] for f in lktree.t_tree_brlen._fields_[n_old:]] == ["n_tot_bl_opt", "bl_opt_evaluations", "bl_opt_status", "bl_opt_host_chain",
                                                                    "bl_opt_on_device"]


def test_a_tree_without_a_device_carries_the_references_defaults():
    capi, lktree = _built()
    t = lktree.LkTree(3, [3, 3, 3], [0, 1, 2], [0.1, 0.1, 0.1], 5, 4, 1)
    try:
        assert t.s_opt.min_diff_lk_local == 1e-3 and t.s_opt.brent_it_max == capi.BRENT_IT_MAX == 1000   # src/init.c:760,770
        assert t.n_tot_bl_opt == 0 and not t.on_device
        assert t.tree.contents.bl_opt_host_chain == 0 and t.tree.contents.bl_opt_status == 0
    finally:
        t.close()


def test_the_bindings_and_the_constants():
    capi, lktree = _built()
    for m in ("optimise_edge_length", "profile_read_edge_length"):
        assert callable(getattr(capi.Instance, m, None)), m
    assert callable(getattr(lktree.LkTree, "Br_Len_Opt", None))
    src = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_brlen.hip")).read()
    assert int(re.search(r"constexpr long long kBrlenMaxPatterns = (\d+);", src).group(1)) == capi.BRLEN_MAX_PATTERNS
    assert int(re.search(r"constexpr int\s+kBrentItMax = (\d+);", src).group(1)) == capi.BRENT_IT_MAX
    m = re.search(r"kBrlenThreads = S == 4 \? (\d+) : (\d+);", src)
    assert {4: int(m.group(1)), 20: int(m.group(2))} == capi.BRLEN_THREADS
    m = re.search(r"kBrlenKeep = S == 4 \? (\d+) : (\d+);", src)
    assert {4: int(m.group(1)), 20: int(m.group(2))} == capi.BRLEN_KEEP
    # the status words of the header are the restatement's
    import brlen_ref
    assert (brlen_ref.SPLINE, brlen_ref.LOWER, brlen_ref.UPPER, brlen_ref.NO_ROOT, brlen_ref.BRACKET, brlen_ref.TOO_LONG, brlen_ref.NAN,
            brlen_ref.CAP) == tuple(range(8))
    step = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_brlen_step.h")).read()
    assert re.search(r"kBrlenSpline = 0, kBrlenLower = 1, kBrlenUpper = 2, kBrlenNoRoot = 3, kBrlenBracket = 4, kBrlenTooLong = 5, "
                     r"kBrlenNaN = 6, kBrlenCap = 7", step)
    # ONE statement of the search's control flow: the kernel and the host layer both compile the step header
    host = open(os.path.join(ROOT, "phyml_amd", "csrc", "host", "phl_lk.c")).read()
    for txt in (src, host):
        assert '#include "' in txt and "phyhip_brlen_step.h" in txt and "brlen_step(&st" in txt and "brlen_begin(&st" in txt
    assert "sqrt(" not in src and "Br_Len_Spline(phydbl" not in host


def test_the_translation_unit_is_in_the_build_list():
    import __graft_entry__ as g
    assert "phyhip_brlen.hip" in dict(g.UNITS)
