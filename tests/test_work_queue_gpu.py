"""Multi-step batches dealt from the work queue (RiemannConfig::work = "queue", riemann.hip
riemann_queue_kernel) on the GPU: every step value of a queue batch is bit for bit the value
the same plan computes under work = "static". A partial depends only on its virtual block,
never on the workgroup that computes it or when, so there is no tolerance anywhere here."""
from __future__ import annotations

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# pi4 fp64 series_exact: 384-sample tiles. The series needs 192 h <= 2e-6, i.e. N >= 96e6.
N_RAGGED = 96_000_001          # 250 000 tiles (not a multiple of 256 lanes) + 1 remainder sample
N_EVEN = 384 * 4096 * 62       # whole rounds at 256 and 4096 lanes, no remainder sample
STEPS = (1, 2, 3, 64)          # batch lengths (run_steps(1) is the fused launch, not a queue
                               # launch: the 1-step queue launch is the 1-step timeline batch)


def _bits(values):
    return [float(v).hex() for v in values]


def _pair(name="pi4", **kw):
    from cuda_v_mpi_amd import Integrator

    q = Integrator(name, work="queue", **kw)
    s = Integrator(name, work="static", **dict(kw, grid=q.plan.grid))
    assert q.plan.multistep and s.plan.multistep
    assert q.plan.work == "queue" and s.plan.work == "static"
    assert q.plan.grid == s.plan.grid and q.plan.block == s.plan.block
    assert q.plan.queue_workgroups >= 1 and s.plan.queue_workgroups == 0
    return q, s


def _batch(it, k, graphs=False):
    it.run_steps(k, pipeline=False, graphs=graphs)
    return [it.plan.host_result(it.plan.host_index_of(j, graphs)) for j in range(k)]


def _same(q, s, k, graphs=False):
    got, want = _batch(q, k, graphs), _batch(s, k, graphs)
    assert len(want) == k and all(math.isfinite(v) for v in want)
    assert _bits(got) == _bits(want), (k, got[:3], want[:3])
    return want


@pytest.mark.parametrize("n", [N_RAGGED, N_EVEN], ids=["ragged", "even"])
@pytest.mark.parametrize("grid", [1, 3, 16])
def test_pi4_series_exact_bitwise(cuda, grid, n):
    """Virtual grids of 1, 3 and 16 at block 256, 1 to 64 steps; with and without the
    exec-masked extra round and the per-point remainder."""
    q, s = _pair(n=n, grid=grid, block=256, slots=64)
    lanes, tiles = grid * 256, n // 384
    ragged = n == N_RAGGED
    assert (tiles % lanes != 0) == (ragged or grid == 3)   # the extra round
    assert (n % 384 != 0) == ragged                        # the remainder sample
    p = q.plan.queue_workgroups
    assert 1 < p <= grid * 64  # never more pullers than a full batch's items; grid 1 has P > 1
    for k in STEPS:
        want = _same(q, s, k)
        assert abs(want[0] - math.pi) < 1e-7
        if k == 1:  # a real 1-step queue launch: the timeline form of the same kernel body
            t = q.timeline(1)
            assert t["work"] == "queue" and _bits(t["values"]) == _bits(want)
    # the plan's P is a full batch's items at most: fewer items than pullers and as many
    # (items > P: test_more_items_than_pullers)
    assert any(k * grid < p for k in STEPS) and any(k * grid == p for k in STEPS)


@pytest.mark.parametrize("n", [N_RAGGED, N_EVEN], ids=["ragged", "even"])
def test_more_items_than_pullers(cuda, n):
    """One puller per CU for a virtual grid of 16 and up to 64 steps: 1024 items for 256
    workgroups, so workgroups run several items each: the item loop's later iterations, the
    seq & 1 alternation of the LDS words, the step count advancing with the claims."""
    q, s = _pair(n=n, grid=16, block=256, slots=64, queue_wg_per_cu=1)
    p = q.plan.queue_workgroups
    assert 1 < p < 64 * 16
    for k in (17, 33, 64):
        assert k * 16 > p  # strictly more items than pullers
        _same(q, s, k)
    k = 64
    want = _batch(s, k)
    t = q.timeline(k)
    assert _bits(t["values"]) == _bits(want)
    own = t["item_owner"].reshape(-1)
    assert (t["item_stamp"] != 0).all() and (own < p).all()
    per_wg = np.bincount(own, minlength=p)
    assert int(per_wg.sum()) == k * 16 and int(per_wg.max()) > 1  # some workgroup ran several
    # such a workgroup's items span more than one step (its step count advanced)
    w = int(per_wg.argmax())
    steps_of_w = np.nonzero((t["item_owner"] == w).any(axis=1))[0]
    print(f"P = {p}, items per workgroup max {per_wg.max()}, workgroup {w} ran steps "
          f"{steps_of_w.min()}..{steps_of_w.max()}")
    assert per_wg.max() >= 3 and len(steps_of_w) > 1


@pytest.mark.parametrize("block", [64, 1024])
def test_blocks_more_items_than_pullers(cuda, block):
    """The same at one wave per workgroup (the next index by readfirstlane) and at sixteen."""
    q, s = _pair(n=N_RAGGED, grid=16, block=block, slots=64, queue_wg_per_cu=1)
    p = q.plan.queue_workgroups
    assert 64 * 16 > p
    for k in (2, 64):
        _same(q, s, k)
    t = q.timeline(64)
    per_wg = np.bincount(t["item_owner"].reshape(-1), minlength=p)
    print(f"block {block}: P = {p}, items per workgroup max {per_wg.max()}")
    assert int(per_wg.sum()) == 64 * 16 and int(per_wg.max()) > 1


@pytest.mark.parametrize("block", [64, 1024])
def test_blocks(cuda, block):
    """One wave per workgroup (no barrier: the claim travels by readfirstlane) and sixteen."""
    q, s = _pair(n=N_RAGGED, grid=3, block=block, slots=8)
    for k in (2, 3, 8):
        _same(q, s, k)


def test_back_to_back_without_a_host_reset(cuda):
    """Batches of 3, 1 and 3 steps on one plan: the last workgroup out re-arms the queue
    words, nothing on the host touches them between launches. (A 1-step batch of a plan is
    the fused launch; the 1-step timeline batch is a 1-step queue launch.)"""
    q, s = _pair(n=N_RAGGED, grid=3, block=256, slots=8)
    a = _same(q, s, 3)
    _same(q, s, 1)
    t = q.timeline(1)
    assert t["work"] == "queue" and _bits(t["values"]) == _bits(a[:1])
    b = _same(q, s, 3)
    assert _bits(a) == _bits(b)


def test_graph_replayed_twice(cuda):
    q, s = _pair(n=N_RAGGED, grid=16, block=256, slots=3)
    a = _same(q, s, 3, graphs=True)
    b = _same(q, s, 3, graphs=True)
    assert q.plan.graphs_ready and q.plan.graph_launches == 2
    assert _bits(a) == _bits(b)
    c = _same(q, s, 6, graphs=True)  # two replays back to back in one call
    assert _bits(c[:3]) == _bits(a)


def test_graphs_of_different_lengths_back_to_back(cuda):
    """Batches of 3, 2, 1 and 3 steps as captured graphs on one plan (a 3-step and a 2-step
    queue graph, the 1-step graph is the fused launch), then 5 = 3 + 2 in one call, each
    replayed with no host reset in between: the queue words re-arm across replays of graphs
    of different lengths."""
    q, s = _pair(n=N_RAGGED, grid=16, block=256, slots=3, queue_wg_per_cu=1)
    first = _same(q, s, 3, graphs=True)
    for k in (2, 1, 3, 5, 2, 3):
        got = _same(q, s, k, graphs=True)
        assert set(_bits(got)) == set(_bits(first))
    assert q.plan.graphs_ready and q.plan.graph_launches == 1 + 1 + 1 + 1 + 2 + 1 + 1


@pytest.mark.parametrize("name,kw", [
    ("table", dict(n=18_000_000)),                 # the LDS / global table tiles, 8-wave hint
    ("pi4", dict(n=4_000_037, dtype="fp32acc")),   # float block sum
    ("sin", dict(n=3_000_003, rule="mid")),
], ids=["table", "fp32acc", "sin"])
def test_other_integrands(cuda, name, kw):
    q, s = _pair(name, slots=8, **kw)
    for k in (2, 5):
        _same(q, s, k)
    if name == "table":  # per-sample tiles stage the table in LDS
        q2, s2 = _pair(name, slots=8, div="ieee", **kw)
        _same(q2, s2, 3)


def test_queue_timeline(cuda):
    """Every item is stamped exactly once, by a workgroup that exists."""
    q, s = _pair(n=N_RAGGED, grid=16, block=256, slots=8)
    k = 5
    want = _batch(s, k)
    t = q.timeline(k)
    p = q.plan.queue_workgroups
    assert t["work"] == "queue" and t["workgroups"] == p and t["grid"] == 16 and t["steps"] == k
    assert _bits(t["values"]) == _bits(want)
    st, own, wg = t["item_stamp"], t["item_owner"], t["wg_stamps"]
    assert st.shape == (k, 16) and own.shape == (k, 16) and wg.shape == (p, 2)
    assert st.dtype == np.uint64 and own.dtype == np.uint32
    assert (st != 0).all() and (own < p).all()          # no sentinel left, owners exist
    assert (wg != 0).all() and (wg[:, 1] >= wg[:, 0]).all()
    assert t["shader_clock"].shape == (p, 2) and t["hw"].shape == (p, 2)
    assert (t["hw"] != 0xFFFFFFFF).all()
    # an item's stamp lies inside its owner's stay, and a workgroup's items are stamped in
    # the order it claimed them (a workgroup's claims only grow)
    flat_st, flat_own = st.reshape(-1), own.reshape(-1)
    assert (flat_st >= wg[flat_own, 0]).all() and (flat_st <= wg[flat_own, 1]).all()
    for w in np.unique(flat_own):
        mine = flat_st[flat_own == w]
        assert (np.diff(mine.astype(np.int64)) >= 0).all()
    assert int(np.bincount(flat_own, minlength=p).sum()) == k * 16
