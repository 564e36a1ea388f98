"""Chained buffers, the host side: a property test of the queue rewriting of the BUILT library (phyhip_queue.hip: defer_forwarded's second pass,
settle_chained, store_definition, devirtualise*) on the CPU.  tests/virt_chain_model.hip is the symbolic model of
tests/virt_defer_model.hip with the chained class switched on (Instance::chain_min_ops): a definition may read buffers that are
unstored themselves.  After every launch the definition of every unstored buffer, evaluated over its inputs' definitions
recursively, is the buffer's plain value; every input of a definition is a tip, stored, or unstored under an older sequence
number; every written buffer is stored or unstored; a reader finds the plain value in memory; the counters match the flags.
Events: replayed post-orders with a matrix per edge, random lists, short lists that write a buffer in the middle of a chain, readers
of a chain's last buffer before any reader of its first (across launches and inside one queue, both orders), readers that rewrite
the queue once without launching it (phyhip_update_eigen_lr's sequence), tip and matrix changes, threshold moves.  No device is touched: the device side of the same contract is tests/test_gpu_chained.py.

Three controls show that the model sees what it is there for: the library rebuilt so that a closure is stored in reverse order, so
that a dependant is kept while the list drops its input's definition, and so that a rewrite that does not launch forgets which
definitions stand in front of the queue, must each fail it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
LIBDIR = os.path.join(ROOT, "phyml_amd", "lib")
CSRC = os.path.join(ROOT, "phyml_amd", "csrc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(os.path.join(LIBDIR, "libphyhip.so"))),
                                reason="needs hipcc and the built library")

HOST_ONLY = ["--offload-arch=gfx950", "-std=c++17", "-O1", "--cuda-host-only", "-w"]
CASES = ((1, 12), (2, 5), (3, 30), (4, 8), (5, 16), (6, 3))  # (seed, tips): the older models'
KEYS = ("launches", "virt_skipped", "in_step", "nostore", "virt_material", "odd", "deferred", "def_material", "def_dropped", "input_writes",
        "replays", "chained", "chain_material", "chain_dropped", "longest_chain", "mid_writes", "end_reads", "double_rewrites")


def compile_host(src, obj, cwd):
    subprocess.run([HIPCC] + HOST_ONLY + ["-c", "-o", obj, src], check=True, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def link(objs, exe, cwd):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-w", "-o", exe] + objs + ["-L" + LIBDIR, "-lphyhip", "-Wl,-rpath," + LIBDIR],
                   check=True, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("virt_chain_model"))
    obj = os.path.join(d, "virt_chain_model.o")
    compile_host(os.path.join(ROOT, "tests", "virt_chain_model.hip"), obj, d)
    exe = os.path.join(d, "virt_chain_model")
    link([obj], exe, d)
    return d, obj, exe


def run(exe, seed, events, tips, soa, in_step=1):
    return subprocess.run([exe, str(seed), str(events), str(tips), str(soa), str(in_step)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=300)


def figures(stdout):
    """the numbers of the model's last line, in its order"""
    return dict(zip(KEYS, (int(x.split()[0]) for x in stdout.split(":")[1].split(","))))


@pytest.mark.parametrize("in_step", [1, 0], ids=["in_step_children", "reissued_children"])
@pytest.mark.parametrize("soa", [1, 0], ids=["nt_two_lane", "aa"])
def test_chained_buffers_keep_the_plain_semantics(model, soa, in_step):
    _, _, exe = model
    total = {}
    for seed, tips in CASES:
        r = run(exe, seed, 3000, tips, soa, in_step)
        assert r.returncode == 0 and "VIRT_CHAIN_MODEL OK" in r.stdout, (seed, tips, r.stdout[-300:], r.stderr[-600:])
        f = figures(r.stdout)
        assert f["launches"] > 1000, r.stdout
        if tips >= 8:  # (fewer tips: hardly ever a list long enough with a chain in it)
            # chaining did occur, chains of three definitions and more, and definitions were both dropped and stored on demand
            assert f["chained"] > 100 and f["chain_dropped"] > 10 and f["chain_material"] > 10 and f["longest_chain"] >= 3, r.stdout
            assert f["mid_writes"] > 5 and f["end_reads"] > 5 and f["double_rewrites"] > 50, r.stdout
        for k, v in f.items():
            total[k] = total.get(k, 0) + v
    # (the older machinery ran beside it)
    assert total["virt_skipped"] > 300 and total["odd"] > 300 and total["deferred"] > 300 and total["def_dropped"] > 50, total


def _variant(model, name, edit):
    """the bookkeeping functions of phyhip_queue.hip with `edit` applied, linked in front of the library"""
    d, obj, _ = model
    src = open(os.path.join(CSRC, "phyhip_queue.hip")).read()
    end = src.index("\n// Host-computed matrices queued")
    head = src[:end].replace('#include "phyhip_host.hpp"', '#include "%s"' % os.path.join(CSRC, "phyhip_host.hpp")) + "\n}\n"
    text = edit(head)
    p = os.path.join(d, name + ".hip")
    open(p, "w").write(text)
    o = os.path.join(d, name + ".o")
    compile_host(p, o, d)
    exe = os.path.join(d, "vcm_" + name)
    link([obj, o], exe, d)
    return exe


def test_the_functions_above_the_cut_as_built_pass(model):
    """The part of phyhip_queue.hip the controls edit, unedited and linked in front of the library: the model passes -- what the
    controls see is their edit."""
    exe = _variant(model, "as_built", lambda head: head)
    for seed in (1, 2, 3):
        r = run(exe, seed, 3000, 12, 1)
        assert r.returncode == 0 and "VIRT_CHAIN_MODEL OK" in r.stdout, (seed, r.stdout[-300:], r.stderr[-600:])


def test_the_model_sees_a_closure_stored_in_reverse_order(model):
    """Control: the definitions in front of the queue in DESCENDING sequence order -- a dependant stored in front of its input."""
    def edit(head):
        order = "I->def_seq[I->pending[at].dest] < I->def_seq[buf]"
        assert head.count(order) == 1
        return head.replace(order, "I->def_seq[I->pending[at].dest] > I->def_seq[buf]")
    exe = _variant(model, "reverse_defect", edit)
    runs = [run(exe, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert all(r.returncode != 0 and "VIRT_CHAIN_MODEL FAIL" in r.stderr for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
    assert any("reads another value than the plain semantics" in r.stderr for r in runs), [r.stderr[-200:] for r in runs]


def test_the_model_sees_a_dependant_kept_over_a_dropped_input(model):
    """Control: settle_chained WITHOUT the rule that stores a definition whose input buffer the list writes -- the dependant stays,
    its input's definition is dropped (or the input is overwritten in memory)."""
    def edit(head):
        rule = "    if (needed || (!dead && (written(I->ddef[b].c1) || written(I->ddef[b].c2)))) m0.push_back(b);\n"
        assert head.count(rule) == 1
        return head.replace(rule, "    if (needed) m0.push_back(b);\n")
    exe = _variant(model, "input_defect", edit)
    runs = [run(exe, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert all(r.returncode != 0 and "VIRT_CHAIN_MODEL FAIL" in r.stderr for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]


def test_the_model_sees_a_rewrite_without_a_launch_that_forgets_the_front(model):
    """Control: rewrite_pending forgets the stored definitions in front of the queue every time it runs.  A reader that rewrites the
    queue without launching it (phyhip_update_eigen_lr) then has the launch's own rewrite take them for ordinary writes of a
    dependant's input and store that dependant at the very front, before its input."""
    def edit(head):
        entry = "  I->pending_inl.clear();\n"
        assert head.count(entry) == 1
        return head.replace(entry, entry + "  I->n_front = 0;\n")
    exe = _variant(model, "front_defect", edit)
    runs = [run(exe, seed, 3000, 12, 1) for seed in (1, 2, 3, 4)]
    assert all(r.returncode != 0 and "VIRT_CHAIN_MODEL FAIL" in r.stderr for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
