"""Parsimony on the device through every layer that needs no GPU: the built library exports the six entry points, both headers declare
the new functions, the host layer exports its own and carries the appended t_tree fields, and the Python bindings expose them.  CPU-only."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("phyhip_set_parsimony", "phyhip_update_partial_parsimony", "phyhip_calculate_edge_parsimony", "phyhip_get_site_parsimony",
         "phyhip_get_partial_parsimony", "phyhip_profile_read_parsimony")
HOST = ("Make_Tree_For_Pars", "Free_Tree_Pars", "Pars", "Update_Partial_Pars", "Post_Order_Pars", "Pre_Order_Pars", "Pars_At_Given_Edge",
        "Update_Pars_At_Given_Edge", "Get_Step_Mat", "Get_Partial_Pars", "Get_Site_Pars")


def _built():
    import __graft_entry__ as g
    g.build()
    from phyml_amd import capi, lktree
    return capi, lktree


def test_the_library_exports_the_entry_points():
    capi, _ = _built()
    L = capi.load()
    for name in ENTRY:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name


def test_the_abi_header_declares_them():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    assert re.search(r"typedef struct \{ int destination, child1, child2; \} phyhip_parsimony_operation;", abi)
    want = {"phyhip_set_parsimony": ("int instance", "int general", "const int *stepMatrix"),
            "phyhip_update_partial_parsimony": ("int instance", "const phyhip_parsimony_operation *ops", "int count"),
            "phyhip_calculate_edge_parsimony": ("int instance", "int buffer1", "int buffer2", "long long *outParsimony"),
            "phyhip_get_site_parsimony": ("int instance", "int *outSitePars"),
            "phyhip_get_partial_parsimony": ("int instance", "int bufferIndex", "int *outUi", "int *outPars", "int *outPPars"),
            "phyhip_profile_read_parsimony": ("int instance", "double *outKernelMs", "int *outLaunches", "double *outPatternUpdates")}
    for name, args in want.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, abi, flags=re.M)
        assert m, name
        got = " ".join(m.group(1).split())
        for a in args:
            assert a in got, (name, a, got)


def test_the_host_header_declares_them_and_the_fields_are_appended():
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    for decl in (r"void Make_Tree_For_Pars\(t_tree \*tree\);", r"void Free_Tree_Pars\(t_tree \*tree\);", r"int  Pars\(t_edge \*b, t_tree \*tree\);",
                 r"void Update_Partial_Pars\(t_tree \*tree, t_edge \*b_fcus, t_node \*n\);", r"void Post_Order_Pars\(t_node \*a, t_node \*d, t_tree \*tree\);",
                 r"void Pre_Order_Pars\(t_node \*a, t_node \*d, t_tree \*tree\);", r"int  Pars_At_Given_Edge\(t_edge \*b, t_tree \*tree\);",
                 r"int  Update_Pars_At_Given_Edge\(t_edge \*b_fcus, t_tree \*tree\);", r"void Get_Step_Mat\(t_tree \*tree\);",
                 r"void Get_Partial_Pars\(t_tree \*tree, t_edge \*b, t_node \*d, int \*ui, int \*pars, int \*p_pars\);",
                 r"void Get_Site_Pars\(t_tree \*tree, int \*site_pars\);"):
        assert re.search("^" + decl, lk, flags=re.M), decl
    body = lk[lk.index("typedef struct __Tree"):lk.index("} t_tree;")]
    order = [body.index(f) for f in ("sh_seed;", "c_pars, best_pars;", "*site_pars;", "general_pars;", "*step_mat;")]
    assert order == sorted(order)   # after everything that was there


def test_the_ctypes_mirror_matches_the_c_struct():
    capi, lktree = _built()
    # the mirror of the appended fields is a ctypes subclass of t_tree: laid out behind sh_seed, every earlier offset as it was
    assert issubclass(lktree.t_tree_pars, lktree.t_tree)
    assert [f[0] for f in lktree.t_tree_pars._fields_[:5]] == ["c_pars", "best_pars", "site_pars", "general_pars", "step_mat"]
    assert lktree.t_tree_pars.c_pars.offset == C.sizeof(lktree.t_tree) == lktree.t_tree.sh_seed.offset + 8
    # the offsets the C compiler gives the appended fields are the mirror's: Get_Step_Mat fills tree->step_mat of a tree without a device
    H = lktree.load()
    for name in HOST:
        assert hasattr(H, name), name
    t = lktree.LkTree(3, [3, 3, 3], [0, 1, 2], [0.1, 0.1, 0.1], 5, 4, 1)
    try:
        assert not t.tree.contents.step_mat
        H.Get_Step_Mat(t.tree)
        import pars_ref
        assert np.array_equal(t.step_mat, pars_ref.nt_step_mat())
        assert t.tree.contents.own_step_mat == 1 and t.tree.contents.c_pars == 0 and not t.tree.contents.site_pars
        H.Free_Tree_Pars(t.tree)
        assert not t.tree.contents.step_mat
    finally:
        t.close()
    t = lktree.LkTree(3, [3, 3, 3], [0, 1, 2], [0.1, 0.1, 0.1], 5, 20, 1)
    try:
        H.Get_Step_Mat(t.tree)
        assert np.array_equal(t.step_mat, 1 - np.eye(20, dtype=np.int64))    # anything but nucleotides: the 0/1 matrix
        H.Free_Tree_Pars(t.tree)
        mine = np.arange(400, dtype=np.int32)
        t.tree.contents.step_mat = mine.ctypes.data_as(C.POINTER(C.c_int))   # a caller-set matrix is left alone
        H.Get_Step_Mat(t.tree)
        assert np.array_equal(t.step_mat.ravel(), np.arange(400)) and t.tree.contents.own_step_mat == 0
        H.Free_Tree_Pars(t.tree)                                              # ... and is not the host layer's to free
        assert np.array_equal(mine, np.arange(400))
    finally:
        t.close()


def test_the_bindings_and_the_constants():
    capi, lktree = _built()
    for m in ("set_parsimony", "update_partial_parsimony", "edge_parsimony", "site_parsimony", "partial_parsimony"):
        assert callable(getattr(capi.Instance, m, None)), m
    for m in ("Make_Tree_For_Pars", "Pars", "Update_Partial_Pars", "Get_Partial_Pars"):
        assert callable(getattr(lktree.LkTree, m, None)), m
    src = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_pars.hip")).read()
    assert int(re.search(r"constexpr int kParsTile = (\d+);", src).group(1)) == capi.PARS_TILE
    assert int(re.search(r"constexpr int kParsStaging = (\d+);", src).group(1)) == capi.PARS_STAGING


def test_the_translation_unit_is_in_the_build_list():
    import __graft_entry__ as g
    assert ("phyhip_pars.hip", []) in g.UNITS
