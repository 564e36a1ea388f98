"""Chained buffers, the host side: a property test of the queue rewriting of the BUILT library (phyhip_unstored.hip: defer_forwarded's
second pass, settle_deferred, store_definition, devirtualise*) on the CPU.  tests/unstored_model.hip run at class 3 (the chained
class switched on, Unstored::chain_min_ops): a definition may read buffers that are unstored themselves.  After every launch the
definition of every unstored buffer, evaluated over its inputs' definitions recursively, is the buffer's plain value; every input
of a definition is a tip, stored, or unstored under an older sequence number; every written buffer is stored or unstored; a reader
finds the plain value in memory; the counters match the classes.  Events: replayed post-orders with a matrix per edge, random lists,
short lists that write a buffer in the middle of a chain, readers of a chain's last buffer before any reader of its first (across
launches and inside one queue, both orders), readers that rewrite the queue once without launching it (phyhip_update_eigen_lr's
sequence), tip and matrix changes, threshold moves.  No device is touched: the device side of the same contract is
tests/test_gpu_chained.py.

Three controls show that the model sees what it is there for: the library rebuilt so that a closure is stored in reverse order, so
that a dependant is kept while the list drops its input's definition, and so that a rewrite that does not launch forgets which
definitions stand in front of the queue, must each fail it."""
import pytest

import unstored_model as um

pytestmark = um.needs_library
CLS = 3


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return um.build(tmp_path_factory.mktemp("virt_chain_model"))


@pytest.mark.parametrize("in_step", [1, 0], ids=["in_step_children", "reissued_children"])
@pytest.mark.parametrize("soa", [1, 0], ids=["nt_two_lane", "aa"])
def test_chained_buffers_keep_the_plain_semantics(model, soa, in_step):
    _, _, exe = model
    total = {}
    for seed, tips in um.CASES:
        r = um.run(exe, CLS, seed, 3000, tips, soa, in_step)
        assert um.passed(r, CLS), (seed, tips, r.stdout[-300:], r.stderr[-600:])
        f = um.figures(r.stdout)
        assert f["launches"] > 1000, r.stdout
        if tips >= 8:  # (fewer tips: hardly ever a list long enough with a chain in it)
            # chaining did occur, chains of three definitions and more, and definitions were both dropped and stored on demand
            assert f["chained"] > 100 and f["chain_dropped"] > 10 and f["chain_material"] > 10 and f["longest_chain"] >= 3, r.stdout
            assert f["mid_writes"] > 5 and f["end_reads"] > 5 and f["double_rewrites"] > 50, r.stdout
        for k, v in f.items():
            total[k] = total.get(k, 0) + v
    # (the older machinery ran beside it)
    assert total["virt_skipped"] > 300 and total["odd"] > 300 and total["deferred"] > 300 and total["def_dropped"] > 50, total


def test_the_functions_above_the_cut_as_built_pass(model):
    """The unit the controls edit, unedited and linked in front of the library: the model passes -- what the controls see is their
    edit.  (The name is from the time the controls cut the bookkeeping out of a larger unit; it is the whole of phyhip_unstored.hip now.)"""
    exe = um.as_built(model)
    for seed in (1, 2, 3, 4):
        r = um.run(exe, CLS, seed, 3000, 12, 1)
        assert um.passed(r, CLS), (seed, r.stdout[-300:], r.stderr[-600:])


def test_the_model_sees_a_closure_stored_in_reverse_order(model):
    """Control: the definitions in front of the queue in DESCENDING sequence order -- a dependant stored in front of its input."""
    exe = um.defect(model, "reverse")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert all(um.failed(r, CLS) for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
    assert any("reads another value than the plain semantics" in r.stderr for r in runs), [r.stderr[-200:] for r in runs]


def test_the_model_sees_a_dependant_kept_over_a_dropped_input(model):
    """Control: settle_deferred WITHOUT the rule that stores a definition whose input buffer the list writes -- the dependant stays,
    its input's definition is dropped (or the input is overwritten in memory)."""
    exe = um.defect(model, "input")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert all(um.failed(r, CLS) for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]


def test_the_model_sees_a_rewrite_without_a_launch_that_forgets_the_front(model):
    """Control: rewrite_pending forgets the stored definitions in front of the queue every time it runs.  A reader that rewrites the
    queue without launching it (phyhip_update_eigen_lr) then has the launch's own rewrite take them for ordinary writes of a
    dependant's input and store that dependant at the very front, before its input."""
    exe = um.defect(model, "front")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3, 4)]
    assert all(um.failed(r, CLS) for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
