"""phyhip_calculate_pairwise_ml_distances through every layer that needs no GPU: the built library exports it, both headers declare
the new functions, the host layer exports its one, the Python bindings expose them, and without a device the documented errors
come back.  CPU-only."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("phyhip_calculate_pairwise_ml_distances", "phyhip_set_pairwise_work_space", "phyhip_profile_read_pairwise")


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
    m = re.search(r"^int phyhip_calculate_pairwise_ml_distances\(([^;]*)\);", abi, flags=re.M)
    assert m, "include/phyhip.h does not declare phyhip_calculate_pairwise_ml_distances"
    args = " ".join(m.group(1).split())
    for a in ("int instance", "int eigenIndex", "int stateFrequenciesIndex", "double minDiffLk", "const double *inInitialDistances",
              "double *outDistances", "double *outInitialDistances", "double *outCounts", "double *outLogLikelihoods", "int *outIterations"):
        assert a in args, (a, args)
    doc = abi[abi.index("ML_Dist (src/lk.c:1783-1906)"):m.start()]
    for must in ("src/lk.c:2416-2473", "src/optimiz.c:1848-1972", "src/utilities.c:2407-2587", "phyhip_set_phyml_options", "host", "libm",
                 "Fill_Missing_Dist", "log_l", "'U'", "inInitialDistances", "PHYHIP_ERROR_NO_IMPLEMENTATION", "PHYHIP_ERROR_OUT_OF_RANGE"):
        assert must in doc, must
    assert re.search(r"^int phyhip_profile_read_pairwise\(int instance, double \*outCountMs, double \*outOptimiseMs, int \*outCalls\);", abi, flags=re.M)
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^void ML_Dist\(t_tree \*tree, phydbl min_diff_lk_local, phydbl \*dist\);", lk, flags=re.M)


def test_the_host_layer_and_the_bindings_expose_them():
    capi, lktree = _built()
    H = lktree.load()
    assert hasattr(H, "ML_Dist")
    for name in ("pairwise_ml_distances", "set_pairwise_work_space", "profile_read_pairwise"):
        assert callable(getattr(capi.Instance, name, None)), name
    assert callable(getattr(lktree.LkTree, "ML_Dist", None))


def test_the_translation_unit_is_in_the_build_list():
    import __graft_entry__ as g
    assert ("phyhip_dist.hip", []) in g.UNITS


def test_the_documented_errors_without_an_instance():
    """The ctypes signature loads and the call refuses what it documents: an instance that does not exist
    (PHYHIP_ERROR_UNINITIALIZED_INSTANCE) and a NULL result matrix (PHYHIP_ERROR_OUT_OF_RANGE) -- neither touches a device."""
    capi, _ = _built()
    L = capi.load()
    fn = L.phyhip_calculate_pairwise_ml_distances
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 6
    fn.restype = C.c_int
    out = np.zeros((2, 2))
    hdr = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    code = lambda name: int(re.search(r"#define %s\s+\((-?\d+)\)" % name, hdr).group(1))
    assert fn(54321, 0, 0, 1e-3, None, out.ctypes.data_as(C.c_void_p), None, None, None, None) == code("PHYHIP_ERROR_UNINITIALIZED_INSTANCE")
    assert b"54321" in L.phyhip_get_last_error()
    assert fn(54321, 0, 0, 1e-3, None, None, None, None, None, None) == code("PHYHIP_ERROR_OUT_OF_RANGE")
    L.phyhip_set_pairwise_work_space.argtypes = [C.c_int, C.c_longlong]
    assert L.phyhip_set_pairwise_work_space(54321, 0) == code("PHYHIP_ERROR_UNINITIALIZED_INSTANCE")
    a, b, n = C.c_double(0), C.c_double(0), C.c_int(0)
    assert L.phyhip_profile_read_pairwise(54321, C.byref(a), C.byref(b), C.byref(n)) == code("PHYHIP_ERROR_UNINITIALIZED_INSTANCE")
