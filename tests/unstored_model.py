"""What the three host-side model tests (test_virt_model.py, test_virt_defer_model.py, test_virt_chain_model.py) share: building
tests/unstored_model.hip against the BUILT library, running it at a class of unstored buffer (1 virtual, 2 + deferred, 3 + chained),
reading the figures of its last line, and building a variant in which the whole of phyml_amd/csrc/phyhip_unstored.hip -- with an
edit applied: a planted defect, or none -- is linked in front of the library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
LIBDIR = os.path.join(ROOT, "phyml_amd", "lib")
CSRC = os.path.join(ROOT, "phyml_amd", "csrc")

needs_library = pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(os.path.join(LIBDIR, "libphyhip.so"))),
                                   reason="needs hipcc and the built library")

HOST_ONLY = ["--offload-arch=gfx950", "-std=c++17", "-O1", "--cuda-host-only", "-w"]
CASES = ((1, 12), (2, 5), (3, 30), (4, 8), (5, 16), (6, 3))  # (seed, tips)
KEYS = ("launches", "virt_skipped", "in_step", "nostore", "virt_material", "odd", "deferred", "def_material", "def_dropped", "input_writes",
        "replays", "chained", "chain_material", "chain_dropped", "longest_chain", "mid_writes", "end_reads", "double_rewrites")


def compile_host(src, obj, cwd):
    subprocess.run([HIPCC] + HOST_ONLY + ["-c", "-o", obj, src], check=True, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def link(objs, exe, cwd):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-w", "-o", exe] + objs + ["-L" + LIBDIR, "-lphyhip", "-Wl,-rpath," + LIBDIR],
                   check=True, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def build(d):
    """the model against the library as built: (directory, the model's object file, the program)"""
    d = str(d)
    obj = os.path.join(d, "unstored_model.o")
    compile_host(os.path.join(ROOT, "tests", "unstored_model.hip"), obj, d)
    exe = os.path.join(d, "unstored_model")
    link([obj], exe, d)
    return d, obj, exe


def run(exe, cls, seed, events, tips, soa, in_step=1):
    return subprocess.run([exe, str(cls), str(seed), str(events), str(tips), str(soa), str(in_step)], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=300)


def passed(r, cls):
    return r.returncode == 0 and "UNSTORED_MODEL OK class %d " % cls in r.stdout


def failed(r, cls):
    return r.returncode != 0 and "UNSTORED_MODEL FAIL (class %d)" % cls in r.stderr


def figures(stdout):
    """the numbers of the model's last line, in its order"""
    return dict(zip(KEYS, (int(x.split()[0]) for x in stdout.split(":")[1].split(","))))


def _variant(model, name, edit):
    """the model with the whole of phyhip_unstored.hip, `edit` applied, linked in front of the library"""
    d, obj, _ = model
    head = open(os.path.join(CSRC, "phyhip_unstored.hip")).read()
    include = '#include "phyhip_host.hpp"'
    assert head.count(include) == 1
    text = edit(head).replace(include, '#include "%s"' % os.path.join(CSRC, "phyhip_host.hpp"))
    p = os.path.join(d, name + ".hip")
    open(p, "w").write(text)
    o = os.path.join(d, name + ".o")
    compile_host(p, o, d)
    exe = os.path.join(d, "um_" + name)
    link([obj, o], exe, d)
    return exe


def replace_once(anchor, new):
    """an edit for _variant: `anchor`, which stands exactly once in the unit, becomes `new`"""
    def edit(head):
        assert head.count(anchor) == 1, anchor
        return head.replace(anchor, new)
    return edit


def as_built(model):
    """the unit unedited, linked in front of the library like a defect: beside it, what a control sees is its edit"""
    d = model[0]
    exe = os.path.join(d, "um_as_built")
    return exe if os.path.exists(exe) else _variant(model, "as_built", lambda head: head)


# The planted defects, each anchored on text that stands exactly once in phyhip_unstored.hip
DEFECTS = {
    # the odd-list fix of rewrite_pending: the first of two re-issued children of an odd list's last reader is not stored
    "pad": replace_once("      d1.pad &= ~kOpNoStore;\n", ""),
    # keep_stored without the keep-real request
    "keep": replace_once("    I->unstored.keep(buf);\n", "    (void)buf;\n"),
    # a short launch that writes a virtual buffer does not make it real
    "stale": replace_once("      if (is_virtual(o.dest)) u.end(o.dest, U::kShortLaunch);\n", "      (void)o;\n"),
    # the settler without the rule that stores a definition whose input buffer the list writes
    "input": replace_once("    if (needed || (!dead && (written(u.def(b).c1) || written(u.def(b).c2)))) m0.push_back(b);\n",
                          "    if (needed) m0.push_back(b);\n"),
    # defer_forwarded without the odd-list rule
    "defer_pad": replace_once("      if (pad_reads_from_memory(win, L.data(), n, i)) continue; // (the odd-list rule, for this class)\n", ""),
    # the definitions in front of the queue in DESCENDING sequence order
    "reverse": replace_once("u.seq(I->pending[at].dest) < u.seq(buf)", "u.seq(I->pending[at].dest) > u.seq(buf)"),
    # rewrite_pending forgets the stored definitions in front of the queue every time it runs
    "front": replace_once("  I->pending_inl.clear();\n", "  I->pending_inl.clear();\n  u.n_front = 0;\n"),
}


def defect(model, name):
    return _variant(model, name + "_defect", DEFECTS[name])
