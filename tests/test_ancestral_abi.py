"""phyhip_calculate_node_state_posteriors through every layer that needs no GPU: the built library exports it, both headers
declare the new functions, the host layer exports its two, and the Python bindings expose them.  CPU-only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    import __graft_entry__ as g
    g.build()
    from phyml_amd import capi, lktree
    return capi, lktree


def test_the_library_exports_the_entry_point():
    capi, _ = _built()
    L = capi.load()
    assert hasattr(L, "phyhip_calculate_node_state_posteriors")
    assert "phyhip_calculate_node_state_posteriors" in capi.SYMBOLS


def test_both_headers_declare_the_new_functions():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    m = re.search(r"^int phyhip_calculate_node_state_posteriors\(([^;]*)\);", abi, flags=re.M)
    assert m, "include/phyhip.h does not declare phyhip_calculate_node_state_posteriors"
    args = " ".join(m.group(1).split())
    for a in ("int instance", "int nodeCount", "const int *sideBufferIndices", "const int *probabilityIndices",
              "const double *inSiteLogLikelihoods", "double *outPosteriors", "int *outNumericalWarning"):
        assert a in args, (a, args)
    assert "bit parity" in abi[abi.index("Ancestral_Sequences_One_Node"):m.start()]   # the header says what is NOT claimed
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^void Get_Ancestral_Probs\(t_tree \*tree, t_node \*d, phydbl \*probs\);", lk, flags=re.M)
    assert re.search(r"^void Get_All_Ancestral_Probs\(t_tree \*tree, phydbl \*probs\);", lk, flags=re.M)


def test_the_host_layer_and_the_bindings_expose_them():
    capi, lktree = _built()
    H = lktree.load()
    assert hasattr(H, "Get_Ancestral_Probs") and hasattr(H, "Get_All_Ancestral_Probs")
    assert callable(getattr(capi.Instance, "node_state_posteriors", None))
    assert callable(getattr(lktree.LkTree, "Ancestral_Probs", None))


def test_the_translation_unit_is_in_the_build_list():
    import __graft_entry__ as g
    assert ("phyhip_ancestral.hip", []) in g.UNITS
