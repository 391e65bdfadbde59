"""cuda_v_mpi_amd — an MI355X-native numerical-integration framework.

Capabilities of the reference (Excalibur1224/Cuda-v-MPI: riemann.cpp, cintegrate.cu,
4main.c, ex4vel.h), rebuilt for AMD Instinct MI355X (gfx950 / CDNA4):

  * Riemann sums of sin(x), 4/(1+x^2), random polynomials and the analytic train model,
    fp64 and packed-fp32, as hand-written HIP kernels with wave64 DPP + LDS reductions;
  * train-profile integration: LDS-staged interpolation of the 1801-point velocity table,
    fused sums, and a single-pass decoupled look-back prefix scan;
  * multi-GPU: one process per GPU, RCCL all-reduce / all-gather over xGMI, hipGraph replay;
  * the reference's CLIs and stdout format (build/bin/{riemann,cintegrate,trainscan,miint}
    and ``python -m cuda_v_mpi_amd``), with --parity emulation of its partition arithmetic;
  * the reference's CPU (MPI) side, native: per-ISA vector kernels on host threads, host
    ranks with rank-order TCP collectives (``backend="host"``, ``--device cpu``,
    ``python -m cuda_v_mpi_amd compare``);
  * any integrand at run time: one C++ expression over x compiled for gfx950 with hipRTC
    (``ops.kernels.riemann_expr``, ``riemann --expr``), and parameter sweeps of it:
    f(x, p0..p7) over K parameter rows per launch (``integrate_expr_sweep``,
    ``riemann --expr ... --params FILE``), and its running integral as a curve: F(x) at
    every sample, or every K-th one, in one call (``integrate_expr_running``,
    ``ops.kernels.riemann_expr_scan``, ``riemann --expr ... --running``), and double
    integrals of f(x, y) over a rectangle (``integrate_expr2d``,
    ``ops.kernels.riemann_expr2d``, ``riemann --expr ... --ya AY --yb BY``), and its
    integral to a requested tolerance with an error estimate, the samples placed where
    the integrand needs them (``integrate_expr_adaptive``, ``ops.kernels.quad_expr``,
    ``riemann --expr ... --rtol R``), and its integral against cos(omega x) or sin(omega x)
    at a cost that does not grow with omega, the Fourier tail on (a, inf) included
    (``integrate_expr_oscillatory``, ``ops.kernels.quad_expr_osc``,
    ``riemann --expr ... --osc cos --omega W --rtol R``), and the same for f(x, p) over K parameter rows, each
    row to its own tolerance in shared rounds (``integrate_expr_adaptive_sweep``,
    ``ops.kernels.quad_expr_sweep``, ``riemann --expr ... --params FILE --row-rtol R``), on a
    shared range or on one range per row, and the running integral F(x_j) on a grid with every
    cell to a tolerance (``integrate_expr_curve``, ``ops.kernels.quad_expr_curve``), and
    the double integral of f(x, y) over a rectangle to a tolerance
    (``integrate_expr2d_adaptive``, ``ops.kernels.quad_expr2d``,
    ``riemann --expr ... --ya AY --yb BY --area-rtol R``) or between two curves, y from
    y_lo(x) to y_hi(x) (``integrate_expr2d_region``, ``ops.kernels.quad_expr2d_region``,
    ``riemann --expr ... --y-lo EXPR --y-hi EXPR --area-rtol R``), and
    its integral over a box in up to 16 variables by
    a randomly shifted lattice rule (``integrate_expr_nd``, ``ops.kernels.lattice_expr``,
    ``riemann --expr ... --box 0:1,0:1,0:3 --m 20``).

Layout: models/ (integrands), ops/ (kernel entry points), parallel/ (decomposition,
process groups), utils/ (fixtures, oracles, output formats), integrate.py (high-level API).
"""
from __future__ import annotations

__version__ = "0.1.0"

from ._native import native, require_gpu  # noqa: F401
from .integrate import IntegrationResult, Integrator, integrate, integrate_expr  # noqa: F401
from .integrate import SweepResult, integrate_expr_sweep  # noqa: F401
from .integrate import RunningResult, integrate_expr_running  # noqa: F401
from .integrate import integrate_expr2d  # noqa: F401
from .integrate import AdaptiveResult, integrate_expr_adaptive  # noqa: F401
from .integrate import AdaptiveSweepResult, integrate_expr_adaptive_sweep  # noqa: F401
from .integrate import CurveResult, integrate_expr_curve  # noqa: F401
from .integrate import OscillatoryResult, integrate_expr_oscillatory  # noqa: F401
from .integrate import Adaptive2DResult, integrate_expr2d_adaptive  # noqa: F401
from .integrate import AdaptiveRegionResult, integrate_expr2d_region  # noqa: F401
from .integrate import LatticeResult, integrate_expr_nd  # noqa: F401
from .models import integrands  # noqa: F401
