"""Exact tests of the table and polynomial Riemann kernels and of the 2-D field kernels: every
value a launch returns is compared with `==` against an integer reference, no tolerance.

With integer table entries / coefficients, h = 2**-k and a dyadic lower limit, every value any
kernel forms — tile midpoints, segment lines and their kinks, Taylor shifts, packed-fp32 pair
sums, lane / wave / block sums, per-workgroup partials, the final h * sum — is a small
multiple of one power of two, so nothing rounds in any order, in fp64 and (for the values the
packed-fp32 paths hold in fp32) in fp32 (cuda_v_mpi_amd/utils/exact_riemann.py). A wrong sign
or offset in a kink, a dropped or doubled tile or remainder sample, a row taken from a
neighbouring slice: each moves the sum by at least one unit and fails here, where the
tolerance tests (test_gpu_kernels.py) and the form-against-form tests (test_gpu_runtime.py)
cannot see it.

The inputs live in riemann_exact_cases.py; test_exact_riemann_cpu.py shows on any box that
each keeps its budget, so a mismatch here is a kernel finding, never an input problem.
Out of reach of the method: sin, pi4, the train velocity and fp32acc have no exact inputs
(sin and the train velocity are held to a 200-bit truth instead: test_trig_truth_gpu.py).
"""
from __future__ import annotations

import pytest
import torch

import riemann_exact_cases as rc
from cuda_v_mpi_amd import Integrator
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.parallel import loopback

pytestmark = pytest.mark.gpu


def _raw(spec, n, c, i0, m) -> float:
    v = kernels.riemann(spec, n, rule=c.rule, dtype=c.dtype, div=c.div, grid=c.grid, i_begin=i0,
                        n_local=m, fused=c.fused)
    return float(v.item())


# ------------------------------------------------------------------------------ table
@pytest.fixture(scope="module")
def table_refs():
    return {c: rc.table_ref(c) for c in rc.TABLE_CASES}


@pytest.mark.parametrize("c", rc.TABLE_CASES, ids=lambda c: c.id)
def test_table_launch_exact(cuda, table_refs, c):
    """Fused and two-kernel launches of the table integrand: segment-line tiles (one-segment,
    kinked, coarse fallback) and per-sample tiles, fp64 and packed fp32, three rules, grids of
    1, 3, 7 and 130 workgroups (all tiles in the extra round, whole rounds plus a remainder
    inside a wave), a tail that is no whole tile, a domain past both ends of the table, and
    rank slices against the reference of their own samples."""
    i0, m = rc.span(c)
    got = _raw(rc.table_spec(c), rc.n_of(c), c, i0, m)
    print(f"{c.id}: got {got!r} want {table_refs[c]!r}")
    assert got == table_refs[c]


def test_second_table_gets_its_own_tensor(cuda):
    """Two specs with different tables on one device, back to back (the device copies are
    cached per table)."""
    a, b = rc.TABLE_CASES[0], rc.TableCase("t2048", 5, "mid", "fp64", "series", 7, True)
    for c in (a, b, a):
        assert _raw(rc.table_spec(c), rc.n_of(c), c, 0, rc.n_of(c)) == rc.table_ref(c)


# ------------------------------------------------------------------------------ plans
def _steps(it, graphs: bool) -> list:
    it.run_steps(rc.PLAN_STEPS, pipeline=True, graphs=graphs)
    if graphs:
        assert it.plan.graphs_ready, it.plan.graph_error
    # the host keeps the last `slots` steps of a batched run (all 8, or the last one)
    kept = range(rc.PLAN_STEPS - min(it.plan.slots, rc.PLAN_STEPS), rc.PLAN_STEPS)
    return [it.plan.host_result(it.plan.host_index_of(k, graphs)) for k in kept]


@pytest.mark.parametrize("graphs", [False, True], ids=["direct", "graphs"])
@pytest.mark.parametrize("block", rc.PLAN_BLOCKS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_table_plan_paths_exact(cuda, dtype, block, graphs):
    """RiemannPlan batches on the table integrand — chained kernels, the multi-step launch
    with its closing kernel, one-step batches — at 5 workgroups of 64, 256 and 1024 threads:
    every step the host keeps of 8 (a batch of 8; the last of the one-step batches) returns
    the reference."""
    c = rc.PLAN_CASES[dtype]
    want = rc.table_ref(c)
    kw = dict(n=rc.n_of(c), rule=c.rule, dtype=dtype, div=c.div, grid=c.grid, block=block)
    chained = Integrator(rc.table_spec(c), slots=rc.PLAN_STEPS, multistep=False, **kw)
    multi = Integrator(rc.table_spec(c), slots=rc.PLAN_STEPS, close="kernel", **kw)
    single = Integrator(rc.table_spec(c), slots=1, **kw)
    assert chained.plan.chained and not chained.plan.multistep
    assert multi.plan.multistep and not multi.plan.close_in_launch
    assert chained.plan.grid == multi.plan.grid == single.plan.grid == c.grid
    assert chained.plan.block == block
    for name, it in (("chained", chained), ("multistep", multi), ("slots1", single)):
        got = _steps(it, graphs)
        print(f"{name} block {block} graphs {graphs}: {got[0]!r} want {want!r}")
        assert got == [want] * min(it.plan.slots, rc.PLAN_STEPS), name


@pytest.mark.parametrize("graphs", [False, True], ids=["direct", "graphs"])
@pytest.mark.parametrize("block", rc.PLAN_BLOCKS)
def test_poly_plan_close_in_launch_exact(cuda, block, graphs):
    """The multi-step launch that closes its batch itself (the table's plans keep the closing
    kernel), on the degree-2 polynomial: 8 steps, each the reference."""
    c = rc.POLY_PLAN_CASE
    it = Integrator(rc.poly_spec(c), n=rc.poly_n(c), rule=c.rule, div=c.div, grid=c.grid,
                    block=block, slots=rc.PLAN_STEPS, close="launch")
    assert it.plan.multistep and it.plan.close_in_launch
    assert _steps(it, graphs) == [rc.poly_ref(c)] * rc.PLAN_STEPS


@pytest.mark.parametrize("world", rc.LOOPBACK_WORLDS)
def test_table_loopback_ranks_exact(cuda, world):
    """W loopback ranks, each its own slice of the table rule: the all-reduced value of every
    rank and step is the whole rule's reference."""
    c = rc.LOOPBACK_CASE
    want, steps = rc.table_ref(c), 5

    def body(rank, comm):
        it = Integrator(rc.table_spec(c), n=rc.n_of(c), rule=c.rule, dtype=c.dtype, div=c.div,
                        comm_obj=comm, slots=4)
        p = it.plan
        assert p.world == world and p.rank == rank and p.collective
        p.prepare_steps(steps)
        p.launch_steps(steps, True, True)
        p.sync()
        assert p.graph_error == ""
        return dict(vals=[p.host_result(p.host_index_of(k, True)) for k in range(1, steps)],
                    begin=p.begin, count=p.count)

    out = loopback.run_ranks(world, body)
    assert sum(o["count"] for o in out) == rc.n_of(c)
    for o in out:
        assert o["vals"] == [want] * (steps - 1)


# ------------------------------------------------------------------------------ polynomial
@pytest.fixture(scope="module")
def poly_refs():
    return {c: rc.poly_ref(c) for c in rc.POLY_CASES}


@pytest.mark.parametrize("c", rc.POLY_CASES, ids=lambda c: c.id)
def test_poly_launch_exact(cuda, poly_refs, c):
    """Integer polynomials: the Taylor-pair tiles (series) and Horner per sample (ieee), fp64
    at degree 2 (k = 10, [-16, 16]) and degree 3 (k = 7, [-8, 8]), packed fp32 at degree 1
    (k = 6, [-64, 64]). The same polynomial with 4, 6, 7, 8 and 9 coefficients (zeros
    appended) runs every coefficient bucket — series 4, 6, 7, 8 wide, Horner 4, 8, 16 wide;
    the zeros exercise the bucket's indexing, not its high-order arithmetic (7 x**7 over
    even one tile at these steps is past the 53-bit budget)."""
    i0, m = rc.poly_span(c)
    v = kernels.riemann(rc.poly_spec(c), rc.poly_n(c), rule=c.rule, dtype=c.dtype, div=c.div,
                        grid=c.grid, i_begin=i0, n_local=m, fused=(c.grid != 3))
    got = float(v.item())
    print(f"{c.id}: got {got!r} want {poly_refs[c]!r}")
    assert got == poly_refs[c]


# ------------------------------------------------------------------------------ 2-D field
def _field(c, cuda):
    T = torch.as_tensor(rc.field(c.tab), dtype=torch.float64, device=cuda).contiguous()
    ny, nx = T.shape
    gx, gy = rc.field_grid(c)
    return T, nx, ny, float(nx - 1), float(ny - 1), gx, gy


@pytest.mark.parametrize("c", rc.FIELD_CASES, ids=lambda c: c.id)
def test_field_whole_and_row_slices_exact(native, cuda, c):
    """The row stream and the tile kernel on integer fields at dyadic sample rates: the whole
    field fused and unfused, and row slices cut at odd rows, each against the reference of
    its own rows (a slice that takes a row from its neighbour fails, even where the
    neighbour gives it up)."""
    T, nx, ny, X, Y, gx, gy = _field(c, cuda)
    assert native.table2d_path(nx, ny, X, Y, gx, gy, 0, gy) == c.path
    want = rc.field_ref(c)
    for fused in (True, False):
        got = float(kernels.table2d(T, X, Y, gx, gy, fused=fused).item())
        print(f"{c.id} fused {fused}: got {got!r} want {want!r}")
        assert got == want, fused
    for j, (r0, r1) in enumerate(rc.field_cuts(gy)):
        got = float(kernels.table2d(T, X, Y, gx, gy, r0, r1, fused=(j % 2 == 0)).item())
        assert got == rc.field_ref(c, r0, r1), (r0, r1)


STREAM_CASES = [c for c in rc.FIELD_CASES if c.path == "stream"]


@pytest.mark.parametrize("c", STREAM_CASES, ids=lambda c: c.id)
def test_field_chained_and_multistep_exact(native, cuda, c):
    """The batch forms Table2DPlan replays, on a caller's integer field (the plan owns its
    field, so its launchers are called directly): chained launches closed by a finalize, and
    the multi-step launch at 1, 3 and 16 step phases with its closing kernel — every
    integration the reference, on the whole field and on a middle row slice."""
    T, nx, ny, X, Y, gx, gy = _field(c, cuda)
    s = torch.cuda.current_stream().cuda_stream
    for r0, r1 in ((0, gy), rc.field_cuts(gy)[1]):
        want = rc.field_ref(c, r0, r1)
        args = (T.data_ptr(), nx, ny, X, Y, gx, gy, r0, r1)
        nb = native.table2d_grid(nx, ny, X, Y, gx, gy, r0, r1)
        # chained: launch j closes launch j - 1, a finalize closes the last
        buf = [torch.empty(nb, dtype=torch.float64, device=cuda) for _ in range(2)]
        out = torch.zeros(3, dtype=torch.float64, device=cuda)
        for j in range(3):
            native.launch_table2d_chained(*args, buf[j & 1].data_ptr(),
                                          buf[(j - 1) & 1].data_ptr() if j else 0,
                                          out[j - 1:].data_ptr() if j else 0, s)
        native.launch_table2d_finalize(buf[0].data_ptr(), nb, out[2:].data_ptr(), s)
        torch.cuda.synchronize()
        assert out.tolist() == [want] * 3, (r0, r1)
        for phases in rc.FIELD_PHASES:
            assert native.table2d_multistep_phases(nx, ny, X, Y, gx, gy, r0, r1, 0,
                                                   rc.FIELD_STEPS, phases) == phases
            parts = torch.empty(rc.FIELD_STEPS * nb, dtype=torch.float64, device=cuda)
            outs = torch.zeros(rc.FIELD_STEPS, dtype=torch.float64, device=cuda)
            native.launch_table2d_multistep(*args, 0, parts.data_ptr(), rc.FIELD_STEPS,
                                            outs.data_ptr(), s, phases)
            torch.cuda.synchronize()
            assert outs.tolist() == [want] * rc.FIELD_STEPS, (r0, r1, phases)
