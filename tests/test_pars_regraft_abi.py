"""The parsimony regraft scan's surface is there: the four C entry points are declared in include/phyhip.h, listed in capi.SYMBOLS
and exported by the built library; the three host-layer names are declared in include/phyhip_lk.h and exported; the slab plan is
stated the same way in capi and in phyhip_scan_plan.hpp.  CPU-only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["phyhip_calculate_regraft_parsimony", "phyhip_get_regraft_site_parsimony", "phyhip_get_regraft_partial_parsimony",
                "phyhip_profile_read_regraft_parsimony"]
HOST_LAYER = ["Pars_Regraft_Scan", "Get_Regraft_Partial_Pars", "Get_Regraft_Site_Pars"]


def _libs():
    import __graft_entry__ as g
    g.build()
    from phyml_amd import capi, lktree
    return capi.load(), capi, lktree.load()


def test_the_four_symbols_are_exported_and_declared():
    L, capi, _ = _libs()
    hdr = open(os.path.join(ROOT, "include", "phyhip.h")).read()
    for s in ENTRY_POINTS:
        assert len(re.findall(r"^int %s\(" % s, hdr, flags=re.M)) == 1, s     # declared once, and named nowhere else in front of a '('
        assert len(re.findall(r"\b%s\s*\(" % s, hdr)) == 1, s
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert "} phyhip_parsimony_candidate;" in hdr
    import ctypes as C
    assert C.sizeof(capi.ParsimonyCandidate) == 12


def test_the_entry_points_enter_as_the_other_scans_do():
    src = open(os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_pars.hip")).read()
    ext = src[src.index('extern "C" {'):]
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"^int (phyhip_[a-z_0-9]+)\(", ext, flags=re.M)]
    bodies = {name: ext[a:b[0]] for (a, name), b in zip(heads, heads[1:] + [(len(ext), None)])}
    for s in ENTRY_POINTS:
        assert s in bodies, s
        assert "kSideQuery" not in bodies[s] and "GET_INST_RES(" not in bodies[s], s
        assert "side_collect(" in bodies[s] or "side_each<kSideDrain, kSideCall>(" in bodies[s], s


def test_the_three_host_layer_names_are_exported():
    _, _, H = _libs()
    hdr = open(os.path.join(ROOT, "include", "phyhip_lk.h")).read()
    for s in HOST_LAYER:
        assert len(re.findall(r"^void %s\(" % s, hdr, flags=re.M)) == 1, s
        assert hasattr(H, s), s
    from phyml_amd import lktree
    assert all(hasattr(lktree.LkTree, s) for s in HOST_LAYER)


def test_the_slab_plan_is_stated_once(tmp_path):
    """capi.pars_regraft_slabs restates ParsScanSlabs, and capi's constants restate the header's: a host compiler builds the plan
    header alone and prints both"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    from phyml_amd import capi
    shapes = [(K, P, cu) for K in (1, 2, 3, 63, 64, 65, 700, 1023, 1024, 1025, 2049, 65535) for P in (1, 256, 257, 382, 2048, 100000)
              for cu in (1, 256)]
    prog = tmp_path / "plan.cpp"
    prog.write_text('#include "%s"\n#include <cstdio>\nusing namespace phyhip_host;\nint main(){\n'
                    'printf("%%d %%zu %%zu\\n", kParsScanSlabFactor, kScanGridCap, sizeof(ParsScanRec));\n%s'
                    'ParsScanLayout f(383, 4, false, 10), g(383, 20, true, 10);\n'
                    'printf("%%zu %%zu %%zu %%zu %%zu %%zu\\n", f.plane_bytes, f.site_bytes, f.total - f.recs, g.plane_bytes, g.recs %% 16, g.sums - g.recs);\n'
                    'return 0;}\n'
                    % (os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_scan_plan.hpp"),
                       "".join('{ParsScanSlabs s(%d, %d, %d); printf("%%zu %%zu\\n", s.count, s.size);}\n' % (K, (P + 255) // 256, cu)
                               for K, P, cu in shapes)))
    exe = tmp_path / "plan"
    subprocess.check_call([cxx, "-std=c++17", "-o", str(exe), str(prog)])
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    assert out[0].split() == [str(capi.PARS_REGRAFT_SLAB_FACTOR), str(capi.PARS_REGRAFT_CHUNK), "16"]
    for line, (K, P, cu) in zip(out[1:], shapes):
        slabs, size = capi.pars_regraft_slabs(K, P, cu)
        assert [int(x) for x in line.split()] == [slabs, size], (K, P, cu)
        assert slabs * size >= K > (slabs - 1) * size and slabs <= K      # every slab but the last is full, none is empty
    # the kept plane (384 patterns: int2 each, or 20 ints each), the kept site scores, 24 bytes a candidate and 8 for each of its two
    # tiles, records 16-byte aligned
    assert [int(x) for x in out[1 + len(shapes)].split()] == [384 * 8, 384 * 4, 10 * (24 + 2 * 8), 20 * 384 * 4, 0, 10 * 16]
    assert capi.pars_regraft_slabs(0, 100, 256) == (0, 0)
