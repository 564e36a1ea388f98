"""phyhip_calculate_sh_support and its companions through every layer that needs no GPU: the built library exports them, both headers
declare the new functions, the host layer exports its three, the Python bindings expose them, and without a device the documented
errors come back.  CPU-only."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("phyhip_set_support_site_log_likelihoods", "phyhip_calculate_sh_support", "phyhip_get_support_alias_table",
       "phyhip_profile_read_support")


def _built():
    import __graft_entry__ as g
    g.build()
    from phyml_amd import capi, lktree
    return capi, lktree


def test_the_library_exports_the_entry_points():
    capi, _ = _built()
    L = capi.load()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in capi.SYMBOLS, s


def test_both_headers_declare_the_new_functions():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    assert re.search(r"^int phyhip_set_support_site_log_likelihoods\(int instance, int slot, const double \*inSiteLogLikelihoods\);", abi, flags=re.M)
    m = re.search(r"^int phyhip_calculate_sh_support\(([^;]*)\);", abi, flags=re.M)
    assert m, "include/phyhip.h does not declare phyhip_calculate_sh_support"
    args = " ".join(m.group(1).split())
    for a in ("int instance", "int siteCount", "int replicateCount", "unsigned long long seed", "double *outSH", "double *outRELL",
              "double *outTotals", "double *outReplicateSums", "int *outAccepted"):
        assert a in args, (a, args)
    doc = abi[abi.index("Statistics_To_SH (src/alrt.c:1148-1298"):m.start()]
    for must in ("src/alrt.c:1091-1140", "src/alrt.c:1184-1216", "src/alrt.c:1254-1287", "src/stats.c:4493-4560", "Philox4x32-10", "(j, 0, r, 0)",
                 ">> 32", "2^-32", "phyhip_set_pattern_weights", "phyhip_get_site_log_likelihoods", "no download", "atomics", "first shard",
                 "PHYHIP_ERROR_NO_IMPLEMENTATION", "PHYHIP_ERROR_OUT_OF_RANGE", "PHYHIP_ERROR_OUT_OF_MEMORY"):
        assert must in doc, must
    assert re.search(r"^int phyhip_get_support_alias_table\(int instance, int siteCount, double \*outProb, int \*outAlias\);", abi, flags=re.M)
    assert re.search(r"^int phyhip_profile_read_support\(int instance, double \*outKernelMs, int \*outCalls\);", abi, flags=re.M)
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^void   Set_Log_Lks_aLRT\(t_tree \*tree, int k\);", lk, flags=re.M)
    assert re.search(r"^phydbl Statistics_To_SH\(t_tree \*tree\);", lk, flags=re.M)
    assert re.search(r"^phydbl Statistics_to_RELL\(t_tree \*tree\);", lk, flags=re.M)
    assert re.search(r"\bint\s+init_len;", lk) and re.search(r"\bunsigned long long sh_seed;", lk)


def test_the_host_layer_and_the_bindings_expose_them():
    capi, lktree = _built()
    H = lktree.load()
    for name in ("Set_Log_Lks_aLRT", "Statistics_To_SH", "Statistics_to_RELL"):
        assert hasattr(H, name), name
        assert callable(getattr(lktree.LkTree, name, None)), name
    for name in ("set_support_site_lnl", "sh_support", "support_alias_table", "profile_read_support"):
        assert callable(getattr(capi.Instance, name, None)), name
    # the Python mirror of t_tree ends with the two new fields, as the C struct does
    assert [f[0] for f in lktree.t_tree._fields_[-2:]] == ["init_len", "sh_seed"]


def test_the_translation_unit_is_in_the_build_list():
    import __graft_entry__ as g
    assert ("phyhip_support.hip", []) in g.UNITS


def test_the_documented_errors_without_an_instance():
    """The ctypes signatures load and the calls refuse an instance that does not exist (PHYHIP_ERROR_UNINITIALIZED_INSTANCE) --
    none of them touches a device."""
    capi, _ = _built()
    L = capi.load()
    hdr = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    code = lambda name: int(re.search(r"#define %s\s+\((-?\d+)\)" % name, hdr).group(1))
    bad = code("PHYHIP_ERROR_UNINITIALIZED_INSTANCE")
    L.phyhip_set_support_site_log_likelihoods.argtypes = [C.c_int, C.c_int, C.c_void_p]
    assert L.phyhip_set_support_site_log_likelihoods(54321, 0, None) == bad
    assert b"54321" in L.phyhip_get_last_error()
    fn = L.phyhip_calculate_sh_support
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 5
    assert fn(54321, 10, 10, 1, None, None, None, None, None) == bad
    L.phyhip_get_support_alias_table.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert L.phyhip_get_support_alias_table(54321, 10, None, None) == bad
    ms, n = C.c_double(0), C.c_int(0)
    assert L.phyhip_profile_read_support(54321, C.byref(ms), C.byref(n)) == bad
