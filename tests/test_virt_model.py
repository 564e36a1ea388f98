"""Virtual buffers, the host side: a property test of the queue rewriting of the BUILT library (phyhip_unstored.hip: rewrite_pending,
devirtualise*) on the CPU.  tests/unstored_model.hip, run at class 1 (the virtual class alone), links libphyhip.so, feeds a hand-built
Instance random queues, evaluations, readers and matrix / tip changes, and follows every rewritten queue with the kernels' forwarding
rules on symbolic values, in lockstep with the plain semantics (every operation stored, in queue order).  No device is touched: the
device side of the same contract is tests/test_gpu_virtual.py.

The controls show that the model sees what it is there for: the library's bookkeeping rebuilt with a planted defect (tests/unstored_model.py)
-- among them the one a real PhyML search found in round 5 (a short launch that rewrites a virtual buffer left its old definition in
force) -- fails it within a few hundred launches, and rebuilt as it stands passes beside each."""
import os

import pytest

import unstored_model as um

pytestmark = um.needs_library
CLS = 1


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return um.build(tmp_path_factory.mktemp("virt_model"))


@pytest.mark.parametrize("soa", [1, 0], ids=["nt_two_lane", "aa"])
def test_rewritten_queues_keep_the_plain_semantics(model, soa):
    _, _, exe = model
    base = int(os.environ.get("PHYHIP_FUZZ_SEED", "0"))
    for seed, tips in um.CASES:
        r = um.run(exe, CLS, base + seed, 3000, tips, soa)
        assert um.passed(r, CLS), (seed, tips, r.stdout[-300:], r.stderr[-600:])
        # ... and the run did exercise the machinery -- and only the virtual class
        f = um.figures(r.stdout)
        assert f["launches"] > 1000 and f["virt_skipped"] > 50 and f["in_step"] > 100, r.stdout
        assert f["deferred"] == 0 and f["chained"] == 0, r.stdout


def test_without_in_step_children(model):
    """Every virtual child re-issued as a non-storing step of its own (the diag build's PHYHIP_VIRT_INLINE=0): two such steps in
    front of the last reader of an odd list put the first of them three steps behind the list's padding re-run."""
    _, _, exe = model
    for seed, tips in ((11, 12), (12, 6), (13, 20)):
        r = um.run(exe, CLS, seed, 3000, tips, 1, in_step=0)
        assert um.passed(r, CLS), (seed, tips, r.stdout[-300:], r.stderr[-600:])
        assert um.figures(r.stdout)["odd"] > 100, r.stdout  # odd lists did occur


def test_the_model_sees_the_unstored_child_of_a_padded_list(model):
    """Control: the rewriting WITHOUT the statement that stores the first of two re-issued children of an odd list's last reader."""
    exe = um.defect(model, "pad")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1, in_step=0) for seed in (11, 12, 13)]
    assert sum(r.returncode != 0 and "re-run of an odd list" in r.stderr for r in runs) >= 2, [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
    assert all(um.passed(um.run(um.as_built(model), CLS, seed, 3000, 12, 1, in_step=0), CLS) for seed in (11, 12, 13))


def test_the_model_sees_a_reader_left_virtual(model):
    """Control: devirtualise() without the keep-real request (round 5's second defect: a long queue that rewrites the buffer with a
    tip x tip operation left it virtual again under the reader that was about to copy it from memory)."""
    exe = um.defect(model, "keep")
    runs = [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3)]
    assert any(um.failed(r, CLS) for r in runs), [(r.stdout[-200:], r.stderr[-200:]) for r in runs]
    assert all(um.passed(um.run(um.as_built(model), CLS, seed, 3000, 12, 1), CLS) for seed in (1, 2, 3))


def test_the_model_sees_a_stale_definition(model):
    """The bookkeeping of phyhip_unstored.hip compiled WITHOUT the statement that makes a buffer real when a short launch rewrites
    it, linked in front of the library: the model must fail -- and pass with the unit as it stands linked in the same way."""
    seen = {name: [um.run(exe, CLS, seed, 3000, 12, 1) for seed in (1, 2, 3)]
            for name, exe in (("as_built", um.as_built(model)), ("defect", um.defect(model, "stale")))}
    assert all(um.passed(r, CLS) for r in seen["as_built"]), seen["as_built"][0].stderr[-400:]
    assert all(um.failed(r, CLS) for r in seen["defect"]), [r.stdout[-200:] for r in seen["defect"]]
