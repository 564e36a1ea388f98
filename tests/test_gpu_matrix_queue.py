"""The queue of transition-matrix refreshes (phyhip_matrix_queue.hpp: device rebuilds queued by phyhip_update_transition_matrices,
uploads queued by phyhip_set_transition_matrix) as the interface shows it: whatever order rebuilds and uploads of a matrix are
queued in, whatever the queue holds in front of them and however long the lists are, every matrix ends as its LAST writer left
it, the buffers are the oracle's, and the evaluation that follows returns the oracle's scalar.

  a. the same matrix written two or three times with no launch asked for in between -- every ordered pair and triple drawn
     from {rebuild(l1), upload(M), rebuild(l2), upload(M')} -- on a quiet queue, behind a queued partial update that reads the
     matrix (the queue is launched on the old value first), and behind a one-sided Lk(NULL) that left buffers unstored (their
     definitions keep the old value: stored first, or moved to a snapshot slot);
  b. one phyhip_update_transition_matrices call of 1, 3, 4, 5, 8, 9, 31, 32, 33 and 69 matrices -- around kArgUp, the fold
     limits 4 and 8, kSmallPm, kEagerPmBatch, and the whole tree -- and lists that name a matrix twice (the second length wins),
     each followed by Lk(b) at an edge of the list;
  c. 69 phyhip_set_transition_matrix calls in a row, one per edge: past the automatic flush at 4 * kUploadBatch = 64.
     (tests/test_gpu_virtual.py::test_a_virtual_buffer_keeps_the_old_matrix_value and tests/test_gpu_chained.py::
     test_a_chain_keeps_its_values_when_matrices_or_tips_change upload every matrix of a tree one call at a time as well, at 57
     and 21 edges: neither reaches 64.)
The command nobody answers (SentCommand, requeue_sent) is driven by tests/test_gpu_resident.py.

What the last writer wrote: a rebuild gives the oracle's update_pmat at the last length; an upload gives the array handed in
-- the oracle's matrix at yet another length, so that the state stays a valid one and a later whole-tree refresh from the
edge lengths agrees on both sides.  Oracle: tests/orc.py, following every call.  36 taxa: 69 edges, a one-sided traversal of
34 operations (more than virt_min_ops = 16).  The pattern count plays no part here: 64 and 32."""
import itertools

import numpy as np
import pytest

import orc
from gpu_common import assert_device_state_is_the_oracles, synthetic_pair

pytestmark = pytest.mark.gpu

SHAPES = {"nt": (36, 64, 4, 4), "nt_c1": (36, 64, 4, 1), "aa": (36, 32, 20, 4)}
SEED = 17
# a: indices into (rebuild(l1), upload(M), rebuild(l2), upload(M'))
SEQUENCES = [s for n in (2, 3) for s in itertools.permutations(range(4), n)]
LIST_LENGTHS = (1, 3, 4, 5, 8, 9, 31, 32, 33, 69)


def _pair(shape, monkeypatch, resident="1"):
    monkeypatch.setenv("PHYHIP_RESIDENT", resident)
    n, P, ns, C = SHAPES[shape]
    t, ot, _, _ = synthetic_pair(n, P, ns, C, seed=SEED, host_pmat=False, ambiguous_every=13)
    assert ot.ne == t.ne == 69 and all(t.edge(e).contents.Pij_rr_idx == e for e in range(t.ne))
    return t, ot


def _matrix_at(ot, l):
    m = ot.m
    return orc.pmat_edge(l, m.ns, m.ncatg, m.gamma_rr, m.br_len_mult, m.l_min, m.l_max, m.r_e_vect, m.l_e_vect, m.e_val)


def _rebuild(t, ot, idx, lens):
    """one phyhip_update_transition_matrices call; the oracle follows the list in order (a matrix named twice: the second length)"""
    t.inst.update_transition_matrices(np.array(idx, np.int32), np.array(lens, np.float64))
    for e, l in zip(idx, lens):
        ot.len[e] = l
        ot.update_pmat(e)
        t.edge(e).contents.l = l


def _upload(t, ot, e, l):
    """one phyhip_set_transition_matrix call with the oracle's matrix at length l"""
    M = _matrix_at(ot, l)
    t.inst.set_transition_matrix(e, M)
    ot.len[e] = l
    ot.pm[e] = M
    t.edge(e).contents.l = l


def _whole_tree(t, ot, both):
    t.Set_Both_Sides(both)
    got, ref = t.Lk(None), ot.lk(None, both_sides=both)
    assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)


def _leave_buffers_unstored(t, ot):
    """a one-sided Lk(NULL): the buffers it writes were all written before (a both-sided traversal), so every buffer of the tree
    stays comparable; all three classes of unstored buffer are there afterwards"""
    _whole_tree(t, ot, False)
    now = (t.inst.virtual_stats()[0], t.inst.deferred_stats()[0], t.inst.chained_stats()[0])
    assert min(now) > 0, now
    return now


def _evaluate(t, ot, b, refresh):
    """refresh: Lk(b), which queues a rebuild of b's matrix at the edge's length first; else the evaluation alone"""
    if refresh:
        return t.Lk(b), ot.lk(b)
    eb = t.edge(b).contents
    child = eb.p_lk_tip_idx if eb.rght.contents.tax else eb.p_lk_rght_idx
    return t.inst.edge_lnl(eb.p_lk_left_idx, child, eb.Pij_rr_idx), ot.edge_lnl(b)


def _check(t, ot, b, what, refresh=False, state_first=False):
    if state_first:
        assert_device_state_is_the_oracles(t, ot, what=what)
    got, ref = _evaluate(t, ot, b, refresh)
    assert_device_state_is_the_oracles(t, ot, what=what)  # (every matrix, bit for bit, as its last writer left it; every buffer)
    print(f"{what}: lnL {got!r} oracle {ref!r}")
    assert np.isfinite(ref) and abs(got - ref) <= 1e-12 * abs(ref), (what, got, ref)
    assert t.inst.numerical_warning() == 0


@pytest.mark.parametrize("resident", ["1", "0"], ids=["resident", "launched"])
@pytest.mark.parametrize("context", ["quiet", "queued_reader", "unstored"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_last_writer_of_a_matrix_wins(shape, context, resident, monkeypatch):
    t, ot = _pair(shape, monkeypatch, resident)
    rng = np.random.default_rng(SEED)
    try:
        _whole_tree(t, ot, True)
        unstored_seen = 0
        for k, seq in enumerate(SEQUENCES):
            e = (5 * k + 3) % ot.ne  # (36 of the 69 edges, pendant and internal)
            lens = [float(v) for v in rng.uniform(0.01, 0.6, 4)]
            if context == "queued_reader":
                # the partial update at an internal end d of edge e, for another edge at d: queued, it reads matrix e
                d = int(ot.el[e] if ot.el[e] >= ot.n else ot.er[e])
                b2 = next(be for (_, be) in ot.adj[d] if be != e)
                t.Update_Partial_Lk(b2, d)
                ot.update_partial(b2, d)  # (on the matrix as it is now)
            elif context == "unstored":
                unstored_seen += sum(_leave_buffers_unstored(t, ot))
            for a in seq:
                if a in (0, 2):
                    _rebuild(t, ot, [e], [lens[a]])
                else:
                    _upload(t, ot, e, lens[a])
            _check(t, ot, e, (shape, context, resident, e, seq))
        assert context != "unstored" or unstored_seen > 0
    finally:
        t.close()


def _lists(ot, rng):
    """[(indices, lengths, b)]: b, an internal edge, is the first of each list"""
    inner = [e for e in range(ot.ne) if ot.el[e] >= ot.n and ot.er[e] >= ot.n]
    out = []
    for i, k in enumerate(LIST_LENGTHS):
        b = inner[(3 * i) % len(inner)]
        idx = [b] + [int(e) for e in rng.permutation(ot.ne) if e != b][:k - 1]
        out.append((idx, [float(v) for v in rng.uniform(0.01, 0.6, k)], b))
    # a matrix named twice, with two lengths: in a short list and in one the device rebuilds at once (33 entries)
    for k in (4, 33):
        idx, lens, b = out[LIST_LENGTHS.index(k - 1)]
        idx, lens = idx + [idx[1]], lens + [float(rng.uniform(0.7, 0.9))]
        idx[0], idx[-2] = idx[-2], idx[0]  # ... and b's own is not the first any more
        lens[0], lens[-2] = lens[-2], lens[0]
        assert len(idx) == k and len(set(idx)) == k - 1 and lens[-1] != lens[idx.index(idx[-1])]
        out.append((idx, lens, b))
    return out


@pytest.mark.parametrize("context", ["quiet", "unstored"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rebuild_lists_around_every_threshold(shape, context, monkeypatch):
    t, ot = _pair(shape, monkeypatch)
    rng = np.random.default_rng(SEED + 1)
    try:
        _whole_tree(t, ot, True)
        for idx, lens, b in _lists(ot, rng):
            if context == "unstored":
                _leave_buffers_unstored(t, ot)
            _rebuild(t, ot, idx, lens)
            _check(t, ot, b, (shape, context, len(idx), len(set(idx))), refresh=True)  # (Lk(b) names b once more: the same length)
    finally:
        t.close()


@pytest.mark.parametrize("context", ["quiet", "unstored"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_uploads_past_the_automatic_flush(shape, context, monkeypatch):
    t, ot = _pair(shape, monkeypatch)
    rng = np.random.default_rng(SEED + 2)
    try:
        _whole_tree(t, ot, True)
        if context == "unstored":
            _leave_buffers_unstored(t, ot)
        for e, l in zip(rng.permutation(ot.ne), rng.uniform(0.01, 0.6, ot.ne)):
            _upload(t, ot, int(e), float(l))
        # every buffer read: the unstored ones are the oracle's on the OLD matrices (the oracle holds them as it computed them),
        # the matrices are the new ones; then an evaluation on the new matrix
        _check(t, ot, ot.root_edge(), (shape, context, "69 uploads"), state_first=True)
    finally:
        t.close()
