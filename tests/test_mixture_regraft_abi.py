"""The mixture regraft scan through every layer that needs no GPU: include/phyhip.h declares the five entry points with the arguments
the issue set, the built library exports them, capi.SYMBOLS lists them and the bindings expose them; the host header declares
MIXT_Lk_Regraft_Scan and the host library exports it; the sizes the bindings repeat are the unit's.  CPU-only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"phyhip_calculate_mixture_regraft_log_likelihoods":
             ("const int *instances", "int count", "const int *eigenIndices", "const phyhip_regraft_candidate *candidates", "int candidateCount",
              "int keepCandidate", "const double *classProba", "const double *rMatWeight", "const double *eFrqWeight", "double rMatWeightSum",
              "double eFrqWeightSum", "double sumProbas", "double *outLogLikelihoods", "int *outWarnings"),
         "phyhip_get_mixture_regraft_partials": ("int firstInstance", "int classIndex", "double *outPartials", "int *outScaleFactors"),
         "phyhip_get_mixture_regraft_transition_matrix": ("int firstInstance", "int classIndex", "int candidate", "int which", "double *outMatrix"),
         "phyhip_set_mixture_regraft_work_space": ("int firstInstance", "long long maxBytes"),
         "phyhip_profile_read_mixture_regraft": ("int firstInstance", "double *outKernelMs", "int *outCalls", "long long *outCandidates")}


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
    assert hasattr(lktree.load(), "MIXT_Lk_Regraft_Scan")


def test_the_abi_header_declares_them():
    abi = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    for name, args in ENTRY.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, abi, flags=re.M)
        assert m, name
        got = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert got == list(args), (name, got)
    # the plain scan's "not built" list no longer names mixtures; it points here
    plain = abi[abi.index("K regraft candidates of one pruned subtree in ONE call"):abi.index("#define PHYHIP_REGRAFT_SUBTREE_IS_LEFT")]
    assert "mixtures." not in plain and "phyhip_calculate_mixture_regraft_log_likelihoods" in plain


def test_the_host_header_declares_the_scan():
    lk = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    assert re.search(r"^void MIXT_Lk_Regraft_Scan\(t_tree \*const \*class_trees, int n_classes, const phydbl \*class_proba, "
                     r"const phydbl \*r_mat_weight,\s*const phydbl \*e_frq_weight, phydbl r_mat_weight_sum, phydbl e_frq_weight_sum, "
                     r"phydbl sum_probas,\s*t_edge \*b_sub, t_node \*d_sub, int link_is_left, phydbl l_sub,\s*"
                     r"int n, t_edge \*const \*b_target, const phydbl \*l_left, const phydbl \*l_rght, phydbl \*lnL\);", lk, flags=re.M)
    assert "no mixture tree\n   type" in lk or "no mixture tree type" in lk


def test_the_bindings_and_the_constants():
    capi, lktree = _built()
    assert callable(getattr(capi, "mixture_regraft_log_likelihoods", None))
    for m in ("mixture_regraft_partials", "mixture_regraft_transition_matrix", "set_mixture_regraft_work_space", "profile_read_mixture_regraft"):
        assert callable(getattr(capi.Instance, m, None)), m
    assert callable(getattr(lktree, "Mixture_Regraft_Scan", None))
    src = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_regraft.hip")).read()
    side = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_side.hpp")).read()
    assert "static_assert(sizeof(MixRegraftClass) == %d" % capi.MIXTURE_REGRAFT_CLASS_BYTES in src
    assert "static_assert(sizeof(MixRegraftHead) == %d" % capi.MIXTURE_REGRAFT_HEAD_BYTES in src
    assert "RegraftUnit mixregraft;" in side and "&I->side->mixregraft.work" in side          # kept on the instance, released with it
    # the work-space arithmetic of the header, as the bindings restate it
    assert capi.mixture_regraft_chunk_candidates(382, 4, 4) >= 512 and capi.mixture_regraft_chunk_candidates(429, 4, 20) >= 512
    K, P, S = 4, 300, 4
    fixed = K * (P * S * 8 + P * 4 + 128) + 200
    per = 3 * K * S * S * 8 + 2 * 8 + 72
    assert capi.mixture_regraft_chunk_candidates(P, K, S, fixed + 5 * per) == 5
    assert capi.mixture_regraft_chunk_candidates(P, K, S, fixed + 5 * per + per // 2) == 5
    assert capi.mixture_regraft_chunk_candidates(P, K, S, 1) == 1
    # no floating-point atomics, no cooperative launch, no new environment switch in the unit
    for word in ("atomicAdd", "hipLaunchCooperativeKernel", "getenv(", "diag_env("):
        for name in ("phyhip_scan_plan.hpp", "phyhip_scan.hpp"):
            assert word not in open(os.path.join(ROOT, "phyml_amd", "csrc", name)).read(), (word, name)
        assert word not in src, word
