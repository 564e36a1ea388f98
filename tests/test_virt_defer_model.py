"""Deferred buffers, the host side: a property test of the queue rewriting of the BUILT library (phyhip_queue.hip: defer_forwarded,
settle_deferred, devirtualise*) on the CPU.  tests/virt_defer_model.hip is the symbolic model of tests/virt_model.hip with
Instance::defer_stores on: definitions may read buffers, and after every launch a deferred definition's inputs are in memory as they
were when it was made, its value is the buffer's plain value, every written buffer is stored, virtual or deferred, a reader finds its
buffer stored and the counters match the flags.  Its events are the older model's plus short lists that write an input of a deferred
buffer and replayed post-order traversals.  No device is touched: the device side of the same contract is tests/test_gpu_deferred.py.

Two controls show that the model sees what it is there for: the library rebuilt without the step that stores a deferred buffer
before one of its inputs is written, and without the odd-list rule for this class, must both fail it."""
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
CASES = ((1, 12), (2, 5), (3, 30), (4, 8), (5, 16), (6, 3))  # (seed, tips): the older model's


def compile_host(src, obj, cwd):
    subprocess.run([HIPCC] + HOST_ONLY + ["-c", "-o", obj, src], check=True, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def link(objs, exe, cwd):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-w", "-o", exe] + objs + ["-L" + LIBDIR, "-lphyhip", "-Wl,-rpath," + LIBDIR],
                   check=True, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("virt_defer_model"))
    obj = os.path.join(d, "virt_defer_model.o")
    compile_host(os.path.join(ROOT, "tests", "virt_defer_model.hip"), obj, d)
    exe = os.path.join(d, "virt_defer_model")
    link([obj], exe, d)
    return d, obj, exe


def run(exe, seed, events, tips, soa, in_step=1):
    return subprocess.run([exe, str(seed), str(events), str(tips), str(soa), str(in_step)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=300)


def figures(stdout):
    """the numbers of the model's last line, in its order"""
    f = stdout.split(":")[1].split(",")
    keys = ("launches", "virt_skipped", "in_step", "nostore", "virt_material", "odd", "deferred", "def_material", "def_dropped", "input_writes", "replays")
    return dict(zip(keys, (int(x.split()[0]) for x in f)))


@pytest.mark.parametrize("in_step", [1, 0], ids=["in_step_children", "reissued_children"])
@pytest.mark.parametrize("soa", [1, 0], ids=["nt_two_lane", "aa"])
def test_deferred_buffers_keep_the_plain_semantics(model, soa, in_step):
    _, _, exe = model
    total = {}
    for seed, tips in CASES:
        r = run(exe, seed, 3000, tips, soa, in_step)
        assert r.returncode == 0 and "VIRT_DEFER_MODEL OK" in r.stdout, (seed, tips, r.stdout[-300:], r.stderr[-600:])
        f = figures(r.stdout)
        assert f["launches"] > 1000, r.stdout
        if tips >= 5:  # (three tips: six internal buffers, hardly ever a list long enough)
            # deferral did occur, and definitions were both dropped and stored on demand
            assert f["deferred"] > 50 and f["def_dropped"] > 10 and f["def_material"] > 10 and f["input_writes"] > 10, r.stdout
        for k, v in f.items():
            total[k] = total.get(k, 0) + v
    assert total["virt_skipped"] > 300 and total["odd"] > 300, total  # (the older machinery ran beside it)


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
    exe = os.path.join(d, "vdm_" + name)
    link([obj, o], exe, d)
    return exe


def test_the_functions_above_the_cut_as_built_pass(model):
    """The part of phyhip_queue.hip the controls edit, unedited and linked in front of the library: the model passes -- what the
    controls see is their edit."""
    exe = _variant(model, "as_built", lambda head: head)
    for seed in (1, 2, 3):
        r = run(exe, seed, 3000, 12, 1)
        assert r.returncode == 0 and "VIRT_DEFER_MODEL OK" in r.stdout, (seed, r.stdout[-300:], r.stderr[-600:])


def test_the_model_sees_an_input_written_under_a_deferred_buffer(model):
    """Control: the rewriting WITHOUT the step that stores a deferred buffer before a list writes one of its inputs."""
    def edit(head):
        step = "    else if (written(I->ddef[b].c1) || written(I->ddef[b].c2)) { stored = true; devirtualise(I, b); } // (an input is written)\n"
        assert step in head
        return head.replace(step, "")
    exe = _variant(model, "input_defect", edit)
    runs = [run(exe, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert all(r.returncode != 0 and "VIRT_DEFER_MODEL FAIL" in r.stderr and "deferred" in r.stderr for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]


def test_the_model_sees_the_deferred_child_of_a_padded_list(model):
    """Control: the rewriting WITHOUT the odd-list rule of the deferred class (the padded re-run of an odd list's last operation
    reads the result three positions back from memory)."""
    def edit(head):
        rule = "    if (i + 3 == n && (pad_read1 == o.dest || pad_read2 == o.dest)) continue; // (the odd-list rule, for this class)\n"
        assert rule in head
        return head.replace(rule, "")
    exe = _variant(model, "pad_defect", edit)
    runs = [run(exe, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert sum(r.returncode != 0 and "re-run of an odd list" in r.stderr for r in runs) >= 2, [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
