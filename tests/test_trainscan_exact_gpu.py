"""The TrainScan class — what the `trainscan` tool and the benchmark run — element by element
and bit for bit against the exact integer reference (cuda_v_mpi_amd/utils/exact_scan.py).

Table: 2048 entries in {-1, 0, 1}; 1024 samples/s for 1500 s = 1 536 000 samples, 375 tiles in
two blocks of 256. Everything is an integer multiple of 2**-10 below 2**53 of them, so the
arrays of every algorithm on every world must equal the reference exactly:
  world 1     fused (the fold variant: no communicator), onepass, lookback
  worlds 2-8  (loopback ranks on one GPU) fused and lookback: every rank's slice of vel and pos,
              i.e. ts_rank_carry, the {T1, T2, count} allgather, exchange_carry and add_carry;
              with replicate, the gathered table
  parity      4main.c's partitions (fill windows of seconds / world whole seconds, slices of
              total / world elements, the residual never scanned), trainscan.cpp:38-47
"""
from __future__ import annotations

import pytest
import torch

import scan_exact_cases as cases
from cuda_v_mpi_amd.parallel import loopback
from cuda_v_mpi_amd.utils import exact_scan as xs
from test_loopback_gpu import native_copy

pytestmark = pytest.mark.gpu
K, SPS, SECONDS, TOTAL = cases.CLASS_K, cases.CLASS_SPS, cases.CLASS_SECONDS, cases.CLASS_TOTAL


@pytest.fixture(scope="module")
def reference(cuda):
    """vel and pos of the whole run as fp64 device tensors; computed once, never modified."""
    assert cases.budget(cases.CLASS) < 53
    ref = xs.exact_scan(cases.table("jag1"), 1, K, 0, TOTAL, device="cuda")
    return xs.to_f64(ref.vel, K), xs.to_f64(ref.pos, K)


def _config(native, **kw):
    c = native.TrainScanConfig()
    c.table = [float(v) for v in cases.table("jag1")]
    c.steps_per_sec = SPS
    c.seconds = SECONDS
    for key, v in kw.items():
        setattr(c, key, v)
    return c


def _arrays(ts, replicate=False):
    """The plan's slice of vel and pos (and the replicated table) as torch tensors."""
    out = {}
    for name, ptr, n in (("vel", ts.velocity_ptr(), ts.local_count),
                         ("pos", ts.position_ptr(), ts.local_count),
                         ("full", ts.replicated_ptr() if replicate else 0, ts.total)):
        if ptr:
            t = torch.empty(n, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            native_copy(t, ptr)
            out[name] = t
    return out


def _run_ranks(native, world, **kw):
    def body(rank, comm):
        ts = native.TrainScan(_config(native, **kw), 0, comm)
        r = ts.run()
        assert r["timeout"] == 0
        return dict(_arrays(ts, kw.get("replicate", False)), r=r, begin=ts.local_begin,
                    count=ts.local_count, algo=ts.algo)
    if world == 1:
        return [body(0, None)]
    return loopback.run_ranks(world, body)


def _same(got, want, what):
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want).flatten()
    i = int(bad[0])
    pytest.fail(f"{what}: {bad.numel()} of {want.numel()} elements differ, first at {i}: "
                f"got {got[i].item()!r}, exact {want[i].item()!r}")


@pytest.mark.parametrize("algo", ["fused", "onepass", "lookback"])
def test_one_gpu_arrays_are_exact(native, reference, algo):
    vel, pos = reference
    (o,) = _run_ranks(native, 1, algo=algo)
    assert o["algo"] == algo and (o["begin"], o["count"]) == (0, TOTAL)
    _same(o["vel"], vel, f"vel [{algo}]")
    _same(o["pos"], pos, f"pos [{algo}]")
    assert o["r"]["distance"] * SPS == vel[-1].item()
    assert o["r"]["sum_of_sums"] == pos[-1].item()


@pytest.mark.parametrize("replicate", [False, True])
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("algo", ["fused", "lookback"])
def test_loopback_rank_slices_are_exact(native, reference, algo, world, replicate):
    vel, pos = reference
    out = _run_ranks(native, world, algo=algo, replicate=replicate)
    assert sum(o["count"] for o in out) == TOTAL
    at = 0
    for r, o in enumerate(out):
        b, n = o["begin"], o["count"]
        assert b == at and o["algo"] == algo
        at += n
        _same(o["vel"], vel[b:b + n], f"vel [{algo}, rank {r} of {world}]")
        _same(o["pos"], pos[b:b + n], f"pos [{algo}, rank {r} of {world}]")
        if replicate:
            _same(o["full"], vel, f"replicated table [{algo}, rank {r} of {world}]")
        assert o["r"]["distance"] * SPS == vel[-1].item()
        assert o["r"]["sum_of_sums"] == pos[-1].item()


def _parity_reference(world):
    """trainscan.cpp:38-47: rank r fills global samples [r fs, (r + 1) fs) with
    fs = (seconds / world) sps, and scans elements [r sub, (r + 1) sub), sub = total / world;
    what a rank's slice holds outside its own fill window is zero. The carries chain the
    slices: rank r starts from the last vel and pos of rank r - 1."""
    sub = TOTAL // world
    fs = (SECONDS // world) * SPS
    c1 = c2 = 0
    vel, pos = [], []
    for r in range(world):
        ref = xs.exact_scan(cases.table("jag1"), 1, K, r * sub, sub, (r * fs, r * fs + fs),
                            (c1, c2), device="cuda")
        c1, c2 = int(ref.vel[-1]), int(ref.pos[-1])
        vel.append(xs.to_f64(ref.vel, K))
        pos.append(xs.to_f64(ref.pos, K))
    return sub, vel, pos


@pytest.mark.parametrize("world", [1, 7])
@pytest.mark.parametrize("algo", ["fused", "lookback"])
def test_parity_partitions_are_exact(native, cuda, algo, world):
    """The arrays only: the printed serial element has its own tests (test_loopback_gpu.py)."""
    assert cases.budget(cases.CLASS) < 53  # bounds every window's subset of the samples
    sub, vel, pos = _parity_reference(world)
    out = _run_ranks(native, world, algo=algo, parity=True)
    for r, o in enumerate(out):
        assert (o["begin"], o["count"]) == (r * sub, sub)
        _same(o["vel"], vel[r], f"vel [{algo}, parity rank {r} of {world}]")
        _same(o["pos"], pos[r], f"pos [{algo}, parity rank {r} of {world}]")
    if world == 7:  # the rule under test leaves a residual and windows short of the slices
        assert TOTAL - world * sub == 4 and (SECONDS // world) * SPS < sub
