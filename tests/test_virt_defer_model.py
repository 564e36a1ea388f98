"""Deferred buffers, the host side: a property test of the queue rewriting of the BUILT library (phyhip_unstored.hip: defer_forwarded,
settle_deferred, devirtualise*) on the CPU.  tests/unstored_model.hip run at class 2 (Unstored::defer_stores on, the chained class
off): definitions may read buffers, and after every launch a deferred definition's inputs are in memory as they were when it was
made, its value is the buffer's plain value, every written buffer is stored, virtual or deferred, a reader finds its buffer stored
and the counters match the classes.  Its events are class 1's plus short lists that write an input of a deferred buffer and replayed
post-order traversals.  No device is touched: the device side of the same contract is tests/test_gpu_deferred.py.

Two controls show that the model sees what it is there for: the library rebuilt without the rule that stores a deferred buffer
before one of its inputs is written, and without the odd-list rule for this class, must both fail it."""
import pytest

import unstored_model as um

pytestmark = um.needs_library
CLS = 2


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return um.build(tmp_path_factory.mktemp("virt_defer_model"))


@pytest.mark.parametrize("in_step", [1, 0], ids=["in_step_children", "reissued_children"])
@pytest.mark.parametrize("soa", [1, 0], ids=["nt_two_lane", "aa"])
def test_deferred_buffers_keep_the_plain_semantics(model, soa, in_step):
    _, _, exe = model
    total = {}
    for seed, tips in um.CASES:
        r = um.run(exe, CLS, seed, 3000, tips, soa, in_step)
        assert um.passed(r, CLS), (seed, tips, r.stdout[-300:], r.stderr[-600:])
        f = um.figures(r.stdout)
        assert f["launches"] > 1000 and f["chained"] == 0, r.stdout
        if tips >= 5:  # (three tips: six internal buffers, hardly ever a list long enough)
            # deferral did occur, and definitions were both dropped and stored on demand
            assert f["deferred"] > 50 and f["def_dropped"] > 10 and f["def_material"] > 10 and f["input_writes"] > 10, r.stdout
        for k, v in f.items():
            total[k] = total.get(k, 0) + v
    assert total["virt_skipped"] > 300 and total["odd"] > 300, total  # (the older machinery ran beside it)


def test_the_functions_above_the_cut_as_built_pass(model):
    """The unit the controls edit, unedited and linked in front of the library: the model passes -- what the controls see is their
    edit.  (The name is from the time the controls cut the bookkeeping out of a larger unit; it is the whole of phyhip_unstored.hip now.)"""
    exe = um.as_built(model)
    for seed in (1, 2, 3):
        r = um.run(exe, CLS, seed, 3000, 12, 1)
        assert um.passed(r, CLS), (seed, r.stdout[-300:], r.stderr[-600:])


def test_the_model_sees_an_input_written_under_a_deferred_buffer(model):
    """Control: the rewriting WITHOUT the rule that stores a deferred buffer before a list writes one of its inputs (the same edit as
    the chained class's control in tests/test_virt_chain_model.py: one settler, one rule)."""
    exe = um.defect(model, "input")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert all(um.failed(r, CLS) and "deferred" in r.stderr for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]


def test_the_model_sees_the_deferred_child_of_a_padded_list(model):
    """Control: the rewriting WITHOUT the odd-list rule of the deferred class (the padded re-run of an odd list's last operation
    reads the result three positions back from memory)."""
    exe = um.defect(model, "defer_pad")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert sum(r.returncode != 0 and "re-run of an odd list" in r.stderr for r in runs) >= 2, [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
