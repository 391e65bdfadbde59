// riemann — Riemann sum of sin(x) on [0, pi] (reference: riemann.cpp, MPI master/worker).
//
// Default output is the reference's two lines (riemann.cpp:92-96):
//   %lf seconds
//   The integral of f(x) from 0.0 to <b> with <n> steps is <sum>      (precision 15)
// Differences by design: every GPU works (the reference's rank 0 only receives, so P
// processes give P-1 workers and P=1 prints 0 — SURVEY B10); the partial sums meet in one
// RCCL all-reduce instead of P-1 MPI_Send/Recv pairs; N is 64-bit (1e10 works, B9).
// --parity runs the master/worker program itself on the GPUs: under P ranks (miintrun -np P,
// torchrun, --gpus P, --loopback P) rank 0 coordinates and integrates nothing, rank r >= 1
// integrates worker r-1's (int)(N/W) samples on its own GPU, the partials meet in one
// allgather and rank 0 adds them in rank order (P=1 -> 0).
//
// Timing: every rank's clock starts after a collective barrier and the reported time is the
// slowest rank's (max over the communicator); --json (or --one-shot) also measures and reports
// ms_one_shot, one integration per call from launch to the result in pinned host memory
// (median). The default program does not: it is the reference's one run.
//
// --device cpu runs the reference's own side of the comparison natively on the host: every
// rank (process) integrates its slice on --threads T vector threads (miint/host.hpp), and
// the ranks' partials meet in a rank-order host all-reduce; --parity emulates --ranks P
// master/worker ranks (riemann.cpp:65-86) in this process.
//
// --expr "EXPR" integrates any f(x) given as one C++ expression over x (HIP device math:
// sin, exp, pow, ...), compiled at run time for gfx950 with hipRTC (miint/expr.hpp) — where
// the reference edits riemann.cpp:37 and recompiles; with --device cpu, compiled for the
// host cores instead (HostExpr). --analytic V adds the error vs V. With --params FILE (one
// row of numbers per line) or --linspace p0=LO:HI:COUNT the expression may also mention
// p0..p7 and every row is integrated in one launch (ExprSweep): one line per row (index,
// parameters, value), or with --json one record carrying rows, nparams and values.
// With --running the expression's running integral is written as a curve (ExprScan): F at
// every sample, or every --every K-th one, to --running-out FILE (raw fp64) or as "x value"
// lines; one rank. With --ya AY --yb BY the expression is over x and y and its double integral
// on [a, b] x [ya, yb] is taken with --n x --ny samples (ExprIntegrator2D, HostExpr2D), the
// ranks splitting the sample rows. With --rtol R and / or --atol T the expression is integrated
// to that tolerance (ExprAdaptive: Gauss-Kronrod (7, 15), bisection where the estimate misses):
// the value, or with --json every field of the result; a warning on stderr when not converged.
// One GPU, one rank: no sample count, rule, sweep, curve, y range or host engine goes with it.
// With a tolerance, --a and --b also take inf, +inf, -inf and infinity (miint/expr.hpp, AdaptRange);
// without one an infinite end is refused.
// With --osc cos|sin --omega W beside --rtol / --atol the expression is integrated against
// cos(W x) or sin(W x) at a cost that does not grow with W (ExprAdaptiveOsc), --b inf being the
// Fourier tail.
// With --params / --linspace and --row-rtol R and / or --row-atol T every row is integrated to
// its own tolerance in shared rounds (ExprAdaptiveSweep): one line per row, or with --json the
// per-row arrays and the call's fields; one warning with the number of rows not converged.
// With --ya / --yb and --area-rtol R and / or --area-atol T the double integral is taken to that
// tolerance (ExprAdaptive2D); with --y-lo EXPR --y-hi EXPR in place of --ya / --yb the limits in
// y are expressions over x (ExprAdaptiveRegion): y between two curves.
// With --box A0:B0,A1:B1,... the expression is over x0, x1, ... and its integral over the box is
// taken by a randomly shifted rank-1 lattice rule (ExprLattice): --m M for the rule of 2^M
// points, or --rtol / --atol for the walk over M; the ranks split the points.
//
//   ./riemann [--n 1e9] [--gpus G] [--integrand sin|pi4|poly|train] [--rule left|mid|right]
//             [--dtype fp64|fp32|fp32acc] [--iters K] [--block 64..1024] [--grid G] [--parity]
//             [--json] [--jsonl FILE]
//             [--device cpu [--threads T] [--ranks P]] [--expr EXPR --a A --b B [--analytic V]]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <vector>

#include "cli_common.hpp"
#include "miint/expr.hpp"
#include "miint/fault.hpp"
#include "miint/host.hpp"
#include "miint/integrator.hpp"
#include "miint/oracle.hpp"
#include "miint/trace.hpp"

using namespace miint;

namespace {

void print_result(double secs, double hi, double nd, double result) {
  std::printf("%lf seconds\n", secs);
  std::cout.precision(15);
  std::cout << "The integral of f(x) from 0.0 to " << hi << " with " << nd << " steps is "
            << result << std::endl;
}

// --device cpu (see the header comment).
int run_host(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  cli::HostRanks hr = cli::host_ranks(a);
  HostPool pool(hr.threads);
  double result = 0.0, host_ms = 0.0;
  int ranks = hr.world;
  if (a.flag("parity")) {
    // riemann.cpp:65-86 as the reference runs it: P ranks -> P-1 workers on host threads,
    // scalar libm sin and sequential sums, rank-order gather; P = 1 -> 0 (B10)
    MIINT_CHECK(hr.world == 1, "--device cpu --parity emulates --ranks P in one process");
    MIINT_CHECK(cfg.integrand == Integrand::kSin && cfg.a == 0.0,
                "--device cpu --parity is the reference's sin on [0, b] program");
    ranks = static_cast<int>(a.integer("ranks", 8));
    MIINT_CHECK(ranks >= 1, "--ranks must be >= 1");
    const double t0 = wall_seconds();
    result = host_riemann_mpi_parity(ranks, nd, cfg.b, pool);
    host_ms = (wall_seconds() - t0) * 1e3;
  } else {
    uint64_t b = 0, c = 0;
    rank_slice(cfg.n, hr.rank, hr.world, &b, &c);
    for (int i = 0; i < iters; ++i) {  // best of --iters
      if (hr.comm) hr.comm->barrier();
      const double t0 = wall_seconds();
      double v = c ? host_riemann(cfg, b, c, pool) : 0.0;
      if (hr.comm) hr.comm->allreduce_sum(&v, 1);
      fault::delay(hr.rank);  // MIINT_FAULT_*: a slow rank (agreement tests)
      const double ms = (wall_seconds() - t0) * 1e3;
      if (i == 0 || ms < host_ms) host_ms = ms;
      result = v;
    }
    if (hr.comm) {  // the slowest rank's time
      double t = -host_ms;
      std::vector<double> all(hr.world);
      hr.comm->allgather(&t, all.data(), 1);
      for (double x : all) host_ms = std::max(host_ms, -x);
    }
  }
  if (hr.rank != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_result(secs, cfg.b, nd, result);
  const double exact = cfg.integrand == Integrand::kTable
                           ? oracle::table_integral(cfg.table, cfg.a, cfg.b)
                           : oracle::analytic(cfg.integrand, cfg.a, cfg.b, cfg.coef, cfg.p0, cfg.p1);
  cli::emit(a, cli::JsonRecord()
                   .add("program", "riemann")
                   .add("device", "cpu")
                   .add("isa", host_isa())
                   .add("integrand", a.str("integrand", "sin"))
                   .add("dtype", "fp64")
                   .add("rule", a.str("rule", "left"))
                   .add("n", nd)
                   .add("ranks", ranks)
                   .add("threads_per_rank", pool.threads())
                   .add("parity", a.flag("parity"))
                   .add("result", result)
                   .add("analytic", exact)
                   .add("abs_err", std::fabs(result - exact))
                   .add("rel_err", std::fabs(result - exact) / std::fabs(exact))
                   .add("host_ms", host_ms)
                   .add("subintervals_per_s", host_ms > 0 ? nd / (host_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

// --expr --device cpu: host ranks, f compiled for the host cores (HostExpr).
int run_host_expr(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  const std::string expr = a.str("expr", "");
  cli::HostRanks hr = cli::host_ranks(a);
  HostPool pool(hr.threads);
  const HostExpr he(expr);
  uint64_t b = 0, c = 0;
  rank_slice(cfg.n, hr.rank, hr.world, &b, &c);
  double result = 0.0, host_ms = 0.0;
  for (int i = 0; i < iters; ++i) {  // best of --iters
    if (hr.comm) hr.comm->barrier();
    const double t0 = wall_seconds();
    double v = c ? he.integrate(cfg.a, cfg.b, cfg.n, cfg.rule, b, c, pool) : 0.0;
    if (hr.comm) hr.comm->allreduce_sum(&v, 1);
    const double ms = (wall_seconds() - t0) * 1e3;
    if (i == 0 || ms < host_ms) host_ms = ms;
    result = v;
  }
  if (hr.rank != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_result(secs, cfg.b, nd, result);
  cli::JsonRecord r;
  r.add("program", "riemann").add("device", "cpu").add("expr", expr).add("a", cfg.a)
      .add("b", cfg.b).add("n", nd).add("rule", a.str("rule", "left")).add("ranks", hr.world)
      .add("threads_per_rank", pool.threads()).add("result", result);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    r.add("analytic", exact).add("abs_err", std::fabs(result - exact));
  }
  cli::emit(a, r.add("host_ms", host_ms)
                   .add("subintervals_per_s", host_ms > 0 ? nd / (host_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

// --expr with --params FILE or --linspace p0=LO:HI:COUNT: a parameter sweep, f(x, p0..p7)
// for every row in one launch (ExprSweep; --device cpu: HostExprSweep). Ranks slice the
// samples, not the rows, and the rows' values meet in one all-reduce.
struct SweepRows {
  std::vector<double> params;  // rows x nparams
  int nparams = 0;
  uint64_t rows = 0;
};

SweepRows sweep_rows(const cli::Args& a) {
  MIINT_CHECK(!(a.has("params") && a.has("linspace")), "give --params FILE or --linspace, not both");
  SweepRows s;
  if (a.has("params")) {
    s.params = load_param_rows(a.str("params", ""), &s.nparams);
  } else {
    s.params = linspace_param_rows(a.str("linspace", ""));
    s.nparams = 1;
  }
  s.rows = s.params.size() / s.nparams;
  return s;
}

void print_sweep(const cli::Args& a, const SweepRows& s, const std::vector<double>& values) {
  if (a.flag("json")) return;  // the record carries the values
  for (uint64_t k = 0; k < s.rows; ++k) {
    std::printf("%llu", static_cast<unsigned long long>(k));
    for (int j = 0; j < s.nparams; ++j) std::printf(" %.17g", s.params[k * s.nparams + j]);
    std::printf(" %.13g\n", values[k]);
  }
}

cli::JsonRecord& add_sweep(cli::JsonRecord& r, const SweepRows& s,
                           const std::vector<double>& values) {
  std::string vs = "[";
  for (size_t k = 0; k < values.size(); ++k) {
    char b[40];
    if (std::isfinite(values[k])) std::snprintf(b, sizeof b, "%s%.17g", k ? "," : "", values[k]);
    else std::snprintf(b, sizeof b, "%snull", k ? "," : "");
    vs += b;
  }
  return r.add("rows", static_cast<int>(s.rows)).add("nparams", s.nparams)
      .add_raw("values", vs + "]");
}

int run_host_expr_sweep(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  const std::string expr = a.str("expr", "");
  const SweepRows sw = sweep_rows(a);
  cli::HostRanks hr = cli::host_ranks(a);
  HostPool pool(hr.threads);
  const HostExprSweep he(expr, sw.nparams);
  uint64_t b = 0, c = 0;
  rank_slice(cfg.n, hr.rank, hr.world, &b, &c);
  std::vector<double> values;
  double host_ms = 0.0;
  for (int i = 0; i < iters; ++i) {  // best of --iters
    if (hr.comm) hr.comm->barrier();
    const double t0 = wall_seconds();
    std::vector<double> v =
        he.integrate(sw.params, sw.rows, cfg.a, cfg.b, cfg.n, cfg.rule, b, c, pool);
    if (hr.comm) hr.comm->allreduce_sum(v.data(), v.size());
    const double ms = (wall_seconds() - t0) * 1e3;
    if (i == 0 || ms < host_ms) host_ms = ms;
    values = v;
  }
  if (hr.rank != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_sweep(a, sw, values);
  cli::JsonRecord r;
  r.add("program", "riemann").add("device", "cpu").add("expr", expr).add("a", cfg.a)
      .add("b", cfg.b).add("n", nd).add("rule", a.str("rule", "left")).add("ranks", hr.world)
      .add("threads_per_rank", pool.threads());
  add_sweep(r, sw, values);
  cli::emit(a, r.add("host_ms", host_ms).add("ms_per_sweep", host_ms)
                   .add("subintervals_per_s",
                        host_ms > 0 ? static_cast<double>(sw.rows) * nd / (host_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

int run_expr_sweep(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  if (cli::on_cpu(a)) return run_host_expr_sweep(a, cfg, nd, iters);
  const std::string expr = a.str("expr", "");
  const SweepRows sw = sweep_rows(a);
  const cli::Topology topo = cli::topology(a);
  std::vector<double> values;
  double dev_ms = 0.0;
  std::mutex mu;
  cli::RankFacts facts;
  cli::run_ranks(topo, [&](int rank, int dev, const Comm* comm) {
    ExprSweep es(expr, sw.nparams, dev, cfg.grid);
    RankAgree agree(comm);
    uint64_t b = 0, c = 0;
    rank_slice(cfg.n, rank, topo.world, &b, &c);
    const std::vector<double> v =
        es.integrate(sw.params, sw.rows, cfg.a, cfg.b, cfg.n, cfg.rule, b, c, 1.0, comm);
    // barrier right before the clock starts; the slowest rank's time
    const double ms = agree.max(es.time(sw.params, sw.rows, cfg.a, cfg.b, cfg.n, cfg.rule, b, c,
                                        iters, [&] { agree.barrier(); },
                                        [&] { fault::delay(rank); }));
    std::lock_guard<std::mutex> g(mu);
    if (rank == topo.rank0) {
      values = v;
      dev_ms = ms;
      facts.note(comm);
    }
  });
  if (topo.rank0 != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_sweep(a, sw, values);
  cli::JsonRecord r;
  r.add("program", "riemann").add("expr", expr).add("a", cfg.a).add("b", cfg.b).add("n", nd)
      .add("rule", a.str("rule", "left")).add("gpus", topo.world);
  add_sweep(r, sw, values);
  facts.add(r, topo);
  cli::emit(a, r.add("device_ms", dev_ms).add("ms_per_sweep", dev_ms)
                   .add("subintervals_per_s",
                        dev_ms > 0 ? static_cast<double>(sw.rows) * nd / (dev_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

// --expr --running: the running integral F_i = h * sum_{j <= i} f(x_j) as a curve (ExprScan),
// every --every K-th value of it. One rank. The values go to --running-out FILE as raw
// little-endian fp64, or to stdout as "x value" lines (at most kRunningMaxLines of them).
constexpr uint64_t kRunningMaxLines = 10000;

int run_expr_running(const cli::Args& a, const RiemannConfig& cfg, double nd) {
  MIINT_CHECK(!a.has("params") && !a.has("linspace"),
              "--running integrates one expression (no --params / --linspace)");
  MIINT_CHECK(!cli::on_cpu(a), "--running has no host engine (--device cpu): it runs on the GPU");
  MIINT_CHECK(!a.has("gpus") && !a.has("loopback") && cli::env_int("WORLD_SIZE", 1) == 1,
              "--running is a one-rank program: no --gpus, --loopback or rank environment "
              "(WORLD_SIZE); slices and rank carries are ExprScan's, through its communicator");
  const std::string expr = a.str("expr", "");
  const long long ev = a.integer("every", 1);
  MIINT_CHECK(ev >= 1, "--every must be >= 1");
  const uint64_t every = static_cast<uint64_t>(ev);
  MIINT_CHECK(cfg.n >= 1, "--running needs --n >= 1");
  const uint64_t outputs = expr_scan_outputs(0, cfg.n, every);
  const std::string path = a.str("running-out", "");
  MIINT_CHECK(!path.empty() || outputs <= kRunningMaxLines,
              "--running would print " + std::to_string(outputs) + " lines (more than " +
                  std::to_string(kRunningMaxLines) + "): thin them with --every K or write raw "
                  "fp64 values with --running-out FILE");
  expr_scan_check(cfg.n, 0, cfg.n, every, outputs);
  MIINT_CHECK(device_count() >= 1, "--running needs a HIP device (no HIP devices visible)");
  set_device(0);
  ExprScan scan(expr, 0);
  DeviceBuffer<double> out(std::max<uint64_t>(outputs, 1));
  const ExprScanResult r =
      scan.run(cfg.a, cfg.b, cfg.n, cfg.rule, 0, cfg.n, every, out.get(), outputs);
  const double h = (cfg.b - cfg.a) / static_cast<double>(cfg.n);
  const uint64_t chunk = 1ull << 22;  // values copied to the host at a time
  std::vector<double> host(std::min<uint64_t>(std::max<uint64_t>(outputs, 1), chunk));
  std::FILE* f = nullptr;
  if (!path.empty()) {
    f = std::fopen(path.c_str(), "wb");
    MIINT_CHECK(f != nullptr, "--running-out: cannot open " + path + " for writing");
  }
  for (uint64_t j0 = 0; j0 < outputs; j0 += chunk) {
    const uint64_t m = std::min<uint64_t>(chunk, outputs - j0);
    MIINT_HIP(hipMemcpy(host.data(), out.get() + j0, m * sizeof(double), hipMemcpyDeviceToHost));
    if (f) {
      if (std::fwrite(host.data(), sizeof(double), m, f) != m) {
        std::fclose(f);
        fail("--running-out: short write to " + path, __FILE__, __LINE__);
      }
    } else {
      for (uint64_t j = 0; j < m; ++j)  // x: the upper limit the value belongs to
        std::printf("%.17g %.17g\n",
                    cfg.a + static_cast<double>(j0 + j + 1) * (static_cast<double>(every) * h),
                    host[j]);
    }
  }
  if (f) MIINT_CHECK(std::fclose(f) == 0, "--running-out: cannot close " + path);
  const double secs = wall_seconds() - process_start_seconds();
  if (f) print_result(secs, cfg.b, nd, r.total);
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr).add("a", cfg.a).add("b", cfg.b).add("n", nd)
      .add("rule", a.str("rule", "left")).add("running", true)
      .add("every", static_cast<double>(every)).add("outputs", static_cast<double>(r.outputs))
      .add("total", r.total);
  if (f) rec.add("running_out", path);
  cli::emit(a, rec.add("device_ms", r.device_ms)
                   .add("subintervals_per_s", r.device_ms > 0 ? nd / (r.device_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

// --expr with --ya AY --yb BY: the double integral of f(x, y) on [a, b] x [ya, yb], n x ny
// samples (--ny, default --n), the same rule on both axes. Ranks split the sample rows.
struct Rule2D {
  double ya = 0.0, yb = 0.0, nyd = 0.0;
  uint64_t ny = 0;
};

Rule2D rule2d(const cli::Args& a, const RiemannConfig& cfg, double nd) {
  MIINT_CHECK(!a.flag("running"), "--running is a curve in x: no --ya / --yb double integral");
  MIINT_CHECK(!a.has("params") && !a.has("linspace"),
              "--ya / --yb integrate one expression over x and y (no --params / --linspace)");
  Rule2D r;
  r.ya = a.num("ya", 0.0);
  r.yb = a.num("yb", 0.0);
  r.nyd = a.num("ny", nd);
  MIINT_CHECK(cfg.n >= 1 && r.nyd >= 1, "--ya / --yb need --n >= 1 and --ny >= 1");
  r.ny = static_cast<uint64_t>(r.nyd);
  return r;
}

void print_result2d(double secs, const RiemannConfig& cfg, const Rule2D& y, double nd,
                    double result) {
  std::printf("%lf seconds\n", secs);
  std::cout.precision(15);
  std::cout << "The integral of f(x, y) over [" << cfg.a << ", " << cfg.b << "] x [" << y.ya
            << ", " << y.yb << "] with " << nd << " x " << y.nyd << " steps is " << result
            << std::endl;
}

cli::JsonRecord record2d(const cli::Args& a, const RiemannConfig& cfg, const Rule2D& y,
                         double nd, double result) {
  cli::JsonRecord r;
  r.add("program", "riemann").add("expr", a.str("expr", "")).add("a", cfg.a).add("b", cfg.b)
      .add("ya", y.ya).add("yb", y.yb).add("n", nd).add("ny", y.nyd)
      .add("rule", a.str("rule", "left")).add("value", result);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    r.add("analytic", exact).add("abs_err", std::fabs(result - exact));
  }
  return r;
}

int run_host_expr2d(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  const Rule2D y = rule2d(a, cfg, nd);
  cli::HostRanks hr = cli::host_ranks(a);
  HostPool pool(hr.threads);
  const HostExpr2D he(a.str("expr", ""));
  uint64_t b = 0, c = 0;
  rank_slice(y.ny, hr.rank, hr.world, &b, &c);
  double result = 0.0, host_ms = 0.0;
  for (int i = 0; i < iters; ++i) {  // best of --iters
    if (hr.comm) hr.comm->barrier();
    const double t0 = wall_seconds();
    double v = he.integrate(cfg.a, cfg.b, cfg.n, y.ya, y.yb, y.ny, cfg.rule, b, c, pool);
    if (hr.comm) hr.comm->allreduce_sum(&v, 1);
    const double ms = (wall_seconds() - t0) * 1e3;
    if (i == 0 || ms < host_ms) host_ms = ms;
    result = v;
  }
  if (hr.rank != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_result2d(secs, cfg, y, nd, result);
  cli::emit(a, record2d(a, cfg, y, nd, result)
                   .add("device", "cpu").add("ranks", hr.world)
                   .add("threads_per_rank", pool.threads()).add("host_ms", host_ms)
                   .add("samples_per_s", host_ms > 0 ? nd * y.nyd / (host_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

int run_expr2d(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  if (cli::on_cpu(a)) return run_host_expr2d(a, cfg, nd, iters);
  const Rule2D y = rule2d(a, cfg, nd);
  const std::string expr = a.str("expr", "");
  const cli::Topology topo = cli::topology(a);
  double result = 0.0, dev_ms = 0.0;
  std::mutex mu;
  cli::RankFacts facts;
  cli::run_ranks(topo, [&](int rank, int dev, const Comm* comm) {
    ExprIntegrator2D ei(expr, dev, cfg.grid);
    RankAgree agree(comm);
    uint64_t b = 0, c = 0;
    rank_slice(y.ny, rank, topo.world, &b, &c);
    const double v =
        ei.integrate(cfg.a, cfg.b, cfg.n, y.ya, y.yb, y.ny, cfg.rule, b, c, 1.0, comm);
    // barrier right before the clock starts; the slowest rank's time
    const double ms = agree.max(ei.time(cfg.a, cfg.b, cfg.n, y.ya, y.yb, y.ny, cfg.rule, b, c,
                                        iters, [&] { agree.barrier(); },
                                        [&] { fault::delay(rank); }));
    std::lock_guard<std::mutex> g(mu);
    if (rank == topo.rank0) {
      result = v;
      dev_ms = ms;
      facts.note(comm);
    }
  });
  if (topo.rank0 != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_result2d(secs, cfg, y, nd, result);
  cli::JsonRecord r = record2d(a, cfg, y, nd, result);
  r.add("gpus", topo.world);
  facts.add(r, topo);
  cli::emit(a, r.add("device_ms", dev_ms)
                   .add("samples_per_s", dev_ms > 0 ? nd * y.nyd / (dev_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

// --expr with --rtol / --atol: the integral to a tolerance (ExprAdaptive). One GPU, one rank.
// A number that does not parse, or a flag of another mode, is refused before any device call.
bool adaptive_requested(const cli::Args& a) { return a.has("rtol") || a.has("atol"); }

double adaptive_number(const cli::Args& a, const std::string& key, double dflt, bool whole) {
  if (!a.has(key)) return dflt;
  const std::string text = a.str(key, "");
  char* end = nullptr;
  const double v = std::strtod(text.c_str(), &end);
  MIINT_CHECK(end != text.c_str() && *end == '\0' && std::isfinite(v) &&
                  (!whole || (v == std::floor(v) && std::fabs(v) < 9.0e15)),
              "--" + key + " must be " + (whole ? "a whole number" : "a number") + " (got '" +
                  text + "')");
  return v;
}

int run_expr_adaptive(const cli::Args& a, const RiemannConfig& cfg) {
  for (const char* k : {"n", "rule", "running", "ya", "yb", "ny", "params", "linspace", "every",
                        "running-out", "loopback"})
    MIINT_CHECK(!a.has(k), std::string("--rtol / --atol choose the samples themselves: --") + k +
                               " does not go with them");
  MIINT_CHECK(a.integer("gpus", 1) <= 1, "--rtol / --atol run on one GPU: --gpus " +
                                             a.str("gpus", "") + " does not go with them (the "
                                             "tolerance would need a collective every round)");
  MIINT_CHECK(cli::env_int("WORLD_SIZE", 1) <= 1,
              "--rtol / --atol run as one rank: a rank environment (WORLD_SIZE = " +
                  std::to_string(cli::env_int("WORLD_SIZE", 1)) + ") does not go with them");
  MIINT_CHECK(!cli::on_cpu(a), "--rtol / --atol have no host engine: --device cpu does not go "
                               "with them");
  AdaptOptions o;
  o.rtol = adaptive_number(a, "rtol", o.rtol, false);
  o.atol = adaptive_number(a, "atol", 0.0, false);
  const double panels = adaptive_number(a, "panels", static_cast<double>(o.panels), true);
  const double depth = adaptive_number(a, "max-depth", o.max_depth, true);
  const double max_iv = adaptive_number(a, "max-intervals", static_cast<double>(o.max_intervals), true);
  MIINT_CHECK(panels >= 0 && max_iv >= 0 && std::fabs(depth) < 1e9,
              "--panels, --max-intervals and --max-depth must not be negative or huge");
  o.panels = static_cast<uint64_t>(panels);
  o.max_depth = static_cast<int>(depth);
  o.max_intervals = static_cast<uint64_t>(max_iv);
  o.unbounded = true;  // an infinity here was typed: --a -inf, --b inf
  adapt_check(cfg.a, cfg.b, o);
  const std::string expr = a.str("expr", "");
  (void)expr_adapt_source(expr);  // a rejected expression: before any device call
  MIINT_CHECK(device_count() >= 1, "--rtol / --atol need a HIP device (no HIP devices visible)");
  set_device(0);
  ExprAdaptive ea(expr, 0);
  const AdaptResult r = ea.integrate(cfg.a, cfg.b, o);
  const double secs = wall_seconds() - process_start_seconds();
  if (!r.converged)
    std::fprintf(stderr, "riemann: not converged: err_est %.3g against tol %.3g (capped %d, "
                 "nonfinite %llu, forced %llu)\n", r.err_est, r.tol, r.capped ? 1 : 0,
                 static_cast<unsigned long long>(r.nonfinite),
                 static_cast<unsigned long long>(r.forced));
  if (!a.flag("json")) std::printf("%.17g\n", r.value);
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr).add("a", cfg.a).add("b", cfg.b)
      .add("rtol", o.rtol).add("atol", o.atol).add("panels", static_cast<double>(o.panels))
      .add("max_depth", o.max_depth).add("max_intervals", static_cast<double>(o.max_intervals))
      .add("value", r.value).add("err_est", r.err_est).add("resabs", r.resabs).add("tol", r.tol)
      .add("converged", r.converged).add("evals", static_cast<double>(r.evals))
      .add("rounds", static_cast<double>(r.rounds))
      .add("intervals", static_cast<double>(r.intervals))
      .add("splits", static_cast<double>(r.splits)).add("floor", static_cast<double>(r.floor))
      .add("forced", static_cast<double>(r.forced))
      .add("nonfinite", static_cast<double>(r.nonfinite)).add("capped", r.capped)
      .add("range", r.range);
  // %.17g round-trips a finite value; a non-finite one prints as null, its bits are here
  char bits[24];
  uint64_t w = 0;
  std::memcpy(&w, &r.value, sizeof w);
  std::snprintf(bits, sizeof bits, "%016llx", static_cast<unsigned long long>(w));
  rec.add("value_bits", bits);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    rec.add("analytic", exact).add("abs_err", std::fabs(r.value - exact));
  }
  cli::emit(a, rec.add("device_ms", r.device_ms).add("seconds_wall", secs));
  return 0;
}

// --expr with --osc cos|sin --omega W and --rtol / --atol: the integral of f(x) cos(W x) or
// f(x) sin(W x) to a tolerance (ExprAdaptiveOsc); --b inf is the Fourier tail. One GPU, one rank.
// Every conflict is refused, named, before any device call.
bool osc_requested(const cli::Args& a) {
  return a.has("osc") || a.has("omega") || a.has("max-cycles");
}

int run_expr_osc(const cli::Args& a, const RiemannConfig& cfg) {
  const std::string who = "--osc / --omega";
  MIINT_CHECK(a.has("osc"), std::string(a.has("omega") ? "--omega" : "--max-cycles") +
                                " belongs to --osc cos|sin (the weight of an oscillatory "
                                "integral): --osc is missing");
  MIINT_CHECK(a.has("omega"), "--osc needs --omega W (the weight is cos(W x) or sin(W x)): "
                              "--omega is missing");
  MIINT_CHECK(a.has("expr"), who + " are the weight of an --expr integrand: --expr is missing");
  MIINT_CHECK(adaptive_requested(a), who + " integrate to a tolerance: they need --rtol R / "
                                           "--atol T");
  for (const char* k : {"n", "rule", "running", "every", "running-out", "ya", "yb", "ny", "y-lo",
                        "y-hi", "box", "params", "linspace", "row-rtol", "row-atol", "area-rtol",
                        "area-atol", "panels-y", "max-total", "m", "shifts", "seed", "z",
                        "periodic", "m-max", "loopback"})
    MIINT_CHECK(!a.has(k), who + " integrate one f(x) against one weight to a tolerance: --" + k +
                               " does not go with them");
  MIINT_CHECK(a.integer("gpus", 1) <= 1, who + " run on one GPU: --gpus " + a.str("gpus", "") +
                                             " does not go with them");
  MIINT_CHECK(cli::env_int("WORLD_SIZE", 1) <= 1,
              who + " run as one rank: a rank environment (WORLD_SIZE = " +
                  std::to_string(cli::env_int("WORLD_SIZE", 1)) + ") does not go with them");
  MIINT_CHECK(!cli::on_cpu(a), who + " have no host engine: --device cpu does not go with them");
  MIINT_CHECK(!(std::isinf(cfg.a) || (std::isinf(cfg.b) && cfg.b < 0.0)),
              who + " take a finite range or (A, inf): --a " + a.str("a", "") + " --b " +
                  a.str("b", "") + " does not go with them ((-inf, b) and two-sided Fourier "
                  "integrals are not supported)");
  const bool tail = std::isinf(cfg.b);
  MIINT_CHECK(tail || !a.has("max-cycles"),
              "--max-cycles bounds the Fourier tail: it needs --b inf");
  MIINT_CHECK(!tail || a.has("atol"),
              "the Fourier tail (--b inf) needs --atol T: its cycles are held to shares of an "
              "absolute tolerance, --rtol alone is refused");
  const OscKind kind = osc_kind(a.str("osc", ""));
  const double omega = adaptive_number(a, "omega", 0.0, false);
  AdaptOptions o;
  OscTailOptions t;
  o.rtol = adaptive_number(a, "rtol", tail ? 0.0 : o.rtol, false);
  o.atol = adaptive_number(a, "atol", 0.0, false);
  const double panels = adaptive_number(
      a, "panels", static_cast<double>(tail ? t.panels : o.panels), true);
  const double depth = adaptive_number(a, "max-depth", o.max_depth, true);
  const double max_iv = adaptive_number(a, "max-intervals", static_cast<double>(o.max_intervals), true);
  const double cycles = adaptive_number(a, "max-cycles", t.max_cycles, true);
  MIINT_CHECK(panels >= 0 && max_iv >= 0 && std::fabs(depth) < 1e9 && std::fabs(cycles) < 1e9,
              "--panels, --max-intervals, --max-depth and --max-cycles must not be negative or "
              "huge");
  (tail ? t.panels : o.panels) = static_cast<uint64_t>(panels);
  o.max_depth = static_cast<int>(depth);
  o.max_intervals = static_cast<uint64_t>(max_iv);
  t.max_cycles = static_cast<int>(cycles);
  osc_check(cfg.a, cfg.b, omega, o, tail, t);
  const std::string expr = a.str("expr", "");
  (void)expr_osc_source(expr);  // a rejected expression: before any device call
  MIINT_CHECK(device_count() >= 1, who + " need a HIP device (no HIP devices visible)");
  set_device(0);
  ExprAdaptiveOsc eo(expr, 0);
  const OscResult r = tail ? eo.integrate_tail(cfg.a, omega, kind, o, t)
                           : eo.integrate(cfg.a, cfg.b, omega, kind, o);
  const double secs = wall_seconds() - process_start_seconds();
  if (!r.converged)
    std::fprintf(stderr, "riemann: not converged: err_est %.3g against tol %.3g: %s\n", r.err_est,
                 r.tol, r.reason.c_str());
  if (!a.flag("json")) std::printf("%.17g\n", r.value);
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr).add("a", cfg.a).add("b", cfg.b)
      .add("omega", omega).add("kind", r.kind)
      .add("rtol", o.rtol).add("atol", o.atol)
      .add("panels", static_cast<double>(tail ? t.panels : o.panels))
      .add("max_depth", o.max_depth).add("max_intervals", static_cast<double>(o.max_intervals))
      .add("value", r.value).add("err_est", r.err_est).add("resabs", r.resabs).add("tol", r.tol)
      .add("converged", r.converged).add("evals", static_cast<double>(r.evals))
      .add("rounds", static_cast<double>(r.rounds))
      .add("intervals", static_cast<double>(r.intervals))
      .add("splits", static_cast<double>(r.splits)).add("floor", static_cast<double>(r.floor))
      .add("forced", static_cast<double>(r.forced))
      .add("nonfinite", static_cast<double>(r.nonfinite)).add("capped", r.capped)
      .add("range", r.range).add("cycles", static_cast<double>(r.cycles))
      .add("extrapolated", r.extrapolated).add("reason", r.reason);
  if (tail) rec.add("max_cycles", t.max_cycles);
  char bits[24];
  uint64_t w = 0;
  std::memcpy(&w, &r.value, sizeof w);
  std::snprintf(bits, sizeof bits, "%016llx", static_cast<unsigned long long>(w));
  rec.add("value_bits", bits);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    rec.add("analytic", exact).add("abs_err", std::fabs(r.value - exact));
  }
  cli::emit(a, rec.add("device_ms", r.device_ms).add("seconds_wall", secs));
  return 0;
}

// --expr with --ya / --yb and --area-rtol / --area-atol: the double integral to a tolerance
// (ExprAdaptive2D). One GPU, one rank. Refusals come before any device call.
bool area_adaptive_requested(const cli::Args& a) {
  return a.has("area-rtol") || a.has("area-atol");
}
bool row_adaptive_requested(const cli::Args& a);
// --y-lo EXPR --y-hi EXPR in place of --ya / --yb: y between two curves (ExprAdaptiveRegion).
bool region_requested(const cli::Args& a) { return a.has("y-lo") || a.has("y-hi"); }

int run_expr_adaptive2d(const cli::Args& a, const RiemannConfig& cfg) {
  const std::string who = "--area-rtol / --area-atol";
  const bool region = region_requested(a);
  MIINT_CHECK(!region || (a.has("y-lo") && a.has("y-hi")),
              "--y-lo and --y-hi go together (the two limits in y of a double integral): --" +
                  std::string(a.has("y-lo") ? "y-hi" : "y-lo") + " is missing");
  MIINT_CHECK(region || (a.has("ya") && a.has("yb")),
              who + " are the tolerance of a double integral: they need --ya AY --yb BY (or "
                    "--y-lo EXPR --y-hi EXPR)");
  MIINT_CHECK(!adaptive_requested(a), who + " are the tolerance of a double integral: --rtol / "
                                            "--atol do not go with them");
  MIINT_CHECK(!row_adaptive_requested(a), who + " are the tolerance of a double integral: "
                                                "--row-rtol / --row-atol do not go with them");
  for (const char* k : {"n", "ny", "rule", "running", "params", "linspace", "every",
                        "running-out", "loopback", "box"})
    MIINT_CHECK(!a.has(k), who + " choose the samples themselves: --" + k +
                               " does not go with them");
  MIINT_CHECK(a.integer("gpus", 1) <= 1, who + " run on one GPU: --gpus " + a.str("gpus", "") +
                                             " does not go with them (the tolerance would need a "
                                             "collective every round)");
  MIINT_CHECK(cli::env_int("WORLD_SIZE", 1) <= 1,
              who + " run as one rank: a rank environment (WORLD_SIZE = " +
                  std::to_string(cli::env_int("WORLD_SIZE", 1)) + ") does not go with them");
  MIINT_CHECK(!cli::on_cpu(a), who + " have no host engine: --device cpu does not go with them");
  Adapt2DOptions o;
  o.rtol = adaptive_number(a, "area-rtol", o.rtol, false);
  o.atol = adaptive_number(a, "area-atol", 0.0, false);
  const double px = adaptive_number(a, "panels", static_cast<double>(o.panels_x), true);
  const double py = adaptive_number(a, "panels-y", px, true);
  const double depth = adaptive_number(a, "max-depth", o.max_depth, true);
  const double max_iv =
      adaptive_number(a, "max-intervals", static_cast<double>(o.max_intervals), true);
  MIINT_CHECK(px >= 0 && py >= 0 && max_iv >= 0 && std::fabs(depth) < 1e9,
              "--panels, --panels-y, --max-intervals and --max-depth must not be negative or "
              "huge");
  o.panels_x = static_cast<uint64_t>(px);
  o.panels_y = static_cast<uint64_t>(py);
  o.max_depth = static_cast<int>(depth);
  o.max_intervals = static_cast<uint64_t>(max_iv);
  // between two curves the rounds run on [a, b] x [0, 1] in (x, v): ya = 0, yb = 1
  const double ya = region ? 0.0 : a.num("ya", 0.0), yb = region ? 1.0 : a.num("yb", 0.0);
  adapt2d_check(cfg.a, cfg.b, ya, yb, o);
  const std::string expr = a.str("expr", "");
  const std::string y_lo = a.str("y-lo", ""), y_hi = a.str("y-hi", "");
  // a rejected expression: before any device call
  if (region) (void)expr_region_source(expr, y_lo, y_hi);
  else (void)expr_adapt2d_source(expr);
  MIINT_CHECK(device_count() >= 1, who + " need a HIP device (no HIP devices visible)");
  set_device(0);
  const Adapt2DResult r = region ? ExprAdaptiveRegion(expr, y_lo, y_hi, 0).integrate(cfg.a, cfg.b, o)
                                 : ExprAdaptive2D(expr, 0).integrate(cfg.a, cfg.b, ya, yb, o);
  const double secs = wall_seconds() - process_start_seconds();
  if (!r.converged)
    std::fprintf(stderr, "riemann: not converged: err_est %.3g against tol %.3g (capped %d, "
                 "nonfinite %llu, forced %llu)\n", r.err_est, r.tol, r.capped ? 1 : 0,
                 static_cast<unsigned long long>(r.nonfinite),
                 static_cast<unsigned long long>(r.forced));
  if (!a.flag("json")) std::printf("%.17g\n", r.value);
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr).add("a", cfg.a).add("b", cfg.b)
      .add("ya", ya).add("yb", yb);
  if (region) rec.add("y_lo", y_lo).add("y_hi", y_hi);
  rec.add("rtol", o.rtol).add("atol", o.atol)
      .add("panels", static_cast<double>(o.panels_x))
      .add("panels_y", static_cast<double>(o.panels_y)).add("max_depth", o.max_depth)
      .add("max_intervals", static_cast<double>(o.max_intervals))
      .add("value", r.value).add("err_est", r.err_est).add("resabs", r.resabs).add("tol", r.tol)
      .add("converged", r.converged).add("evals", static_cast<double>(r.evals))
      .add("rounds", static_cast<double>(r.rounds))
      .add("intervals", static_cast<double>(r.intervals))
      .add("splits", static_cast<double>(r.splits))
      .add("splits_x", static_cast<double>(r.splits_x))
      .add("splits_y", static_cast<double>(r.splits_y))
      .add("floor", static_cast<double>(r.floor)).add("forced", static_cast<double>(r.forced))
      .add("nonfinite", static_cast<double>(r.nonfinite)).add("capped", r.capped);
  // %.17g round-trips a finite value; a non-finite one prints as null, its bits are here
  char bits[24];
  uint64_t w = 0;
  std::memcpy(&w, &r.value, sizeof w);
  std::snprintf(bits, sizeof bits, "%016llx", static_cast<unsigned long long>(w));
  rec.add("value_bits", bits);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    rec.add("analytic", exact).add("abs_err", std::fabs(r.value - exact));
  }
  cli::emit(a, rec.add("device_ms", r.device_ms).add("seconds_wall", secs));
  return 0;
}

// Arrays of a --json record. %.17g round-trips a finite value; a non-finite one prints as null,
// its bits are in the record's value_bits.
std::string json_doubles(const std::vector<double>& v) {
  std::string s = "[";
  for (size_t k = 0; k < v.size(); ++k) {
    char b[40];
    if (std::isfinite(v[k])) std::snprintf(b, sizeof b, "%s%.17g", k ? "," : "", v[k]);
    else std::snprintf(b, sizeof b, "%snull", k ? "," : "");
    s += b;
  }
  return s + "]";
}
std::string json_counts(const std::vector<uint64_t>& v) {
  std::string s = "[";
  for (size_t k = 0; k < v.size(); ++k)
    s += (k ? "," : "") + std::to_string(static_cast<unsigned long long>(v[k]));
  return s + "]";
}
std::string json_flags(const std::vector<uint8_t>& v) {
  std::string s = "[";
  for (size_t k = 0; k < v.size(); ++k) s += std::string(k ? "," : "") + (v[k] ? "true" : "false");
  return s + "]";
}
std::string json_bits(const std::vector<double>& v) {
  std::string bits = "[";
  for (size_t k = 0; k < v.size(); ++k) {
    char b[24];
    uint64_t w = 0;
    std::memcpy(&w, &v[k], sizeof w);
    std::snprintf(b, sizeof b, "%s\"%016llx\"", k ? "," : "", static_cast<unsigned long long>(w));
    bits += b;
  }
  return bits + "]";
}

// The lines of a text file, `columns` numbers each, row-major (blank lines and lines that begin
// with # are skipped); anything else is refused, naming the line.
std::vector<double> load_columns(const std::string& path, int columns, const std::string& flag,
                                 const std::string& what) {
  std::FILE* f = std::fopen(path.c_str(), "r");
  MIINT_CHECK(f != nullptr, flag + " " + path + ": cannot open the file");
  std::vector<double> out;
  char line[512];
  for (int n = 1; std::fgets(line, sizeof line, f); ++n) {
    const char* s = line;
    while (*s == ' ' || *s == '\t') ++s;
    if (*s == '\0' || *s == '\n' || *s == '\r' || *s == '#') continue;
    int got = 0;
    bool ok = true;
    for (;;) {
      char* end = nullptr;
      const double v = std::strtod(s, &end);
      if (end == s) break;
      if (++got <= columns) out.push_back(v);
      s = end;
    }
    while (*s == ' ' || *s == '\t' || *s == '\n' || *s == '\r') ++s;
    ok = got == columns && *s == '\0';
    if (!ok) {
      std::fclose(f);
      std::string text(line);
      while (!text.empty() && (text.back() == '\n' || text.back() == '\r')) text.pop_back();
      fail(flag + " " + path + ": line " + std::to_string(n) + ": expected `" + what +
               "`, got '" + text + "'", __FILE__, __LINE__);
    }
  }
  std::fclose(f);
  return out;
}

// --expr with --params / --linspace and --row-rtol / --row-atol: every row to its own tolerance
// in shared rounds (ExprAdaptiveSweep), on the shared [--a, --b] or, with --ranges FILE, on a
// range per row. One GPU, one rank. Refusals come before any device call.
bool row_adaptive_requested(const cli::Args& a) { return a.has("row-rtol") || a.has("row-atol"); }

int run_expr_adaptive_sweep(const cli::Args& a, const RiemannConfig& cfg) {
  const std::string who = "--row-rtol / --row-atol";
  MIINT_CHECK(!adaptive_requested(a), who + " are the per-row tolerance of a parameter sweep: "
                                            "--rtol / --atol do not go with them");
  for (const char* k : {"n", "rule", "running", "ya", "yb", "ny", "every", "running-out",
                        "loopback", "box"})
    MIINT_CHECK(!a.has(k), who + " choose the samples themselves: --" + k +
                               " does not go with them");
  MIINT_CHECK(a.has("params") || a.has("linspace"),
              who + " need the rows of --params FILE or --linspace p0=LO:HI:COUNT");
  MIINT_CHECK(a.integer("gpus", 1) <= 1, who + " run on one GPU: --gpus " + a.str("gpus", "") +
                                             " does not go with them (the tolerances would need "
                                             "a collective every round)");
  MIINT_CHECK(cli::env_int("WORLD_SIZE", 1) <= 1,
              who + " run as one rank: a rank environment (WORLD_SIZE = " +
                  std::to_string(cli::env_int("WORLD_SIZE", 1)) + ") does not go with them");
  MIINT_CHECK(!cli::on_cpu(a), who + " have no host engine: --device cpu does not go with them");
  AdaptSweepOptions o;
  o.rtol = adaptive_number(a, "row-rtol", o.rtol, false);
  o.atol = adaptive_number(a, "row-atol", 0.0, false);
  const double panels = adaptive_number(a, "panels", 0.0, true);
  const double depth = adaptive_number(a, "max-depth", o.max_depth, true);
  const double max_iv = adaptive_number(a, "max-intervals", 0.0, true);
  const double max_total = adaptive_number(a, "max-total", static_cast<double>(o.max_total), true);
  MIINT_CHECK(panels >= 0 && max_iv >= 0 && max_total >= 0 && std::fabs(depth) < 1e9,
              "--panels, --max-intervals, --max-total and --max-depth must not be negative or "
              "huge");
  o.panels = static_cast<uint64_t>(panels);
  o.max_depth = static_cast<int>(depth);
  o.max_intervals = static_cast<uint64_t>(max_iv);
  o.max_total = static_cast<uint64_t>(max_total);
  const bool ranged = a.has("ranges");
  MIINT_CHECK(!ranged || !(a.has("a") || a.has("b")),
              "--ranges gives every row its own a and b: --a / --b do not go with it");
  o.unbounded = !ranged;  // an infinity here was typed: --a -inf, --b inf
  const SweepRows sw = sweep_rows(a);
  std::vector<double> lo, hi;  // --ranges FILE: K lines `a b`
  if (ranged) {
    const std::string path = a.str("ranges", "");
    const std::vector<double> ends = load_columns(path, 2, "--ranges", "a b");
    MIINT_CHECK(ends.size() == 2 * sw.rows,
                "--ranges " + path + ": " + std::to_string(ends.size() / 2) + " ranges for " +
                    std::to_string(sw.rows) + " rows");
    for (uint64_t k = 0; k < sw.rows; ++k) {
      lo.push_back(ends[2 * k]);
      hi.push_back(ends[2 * k + 1]);
    }
  }
  const AdaptSweepOptions used =
      ranged ? adapt_sweep_ranges_check(sw.rows, sw.nparams, sw.params.size(), lo, hi, o)
             : adapt_sweep_check(sw.rows, sw.nparams, sw.params.size(), cfg.a, cfg.b, o);
  const std::string expr = a.str("expr", "");
  (void)expr_adapt_sweep_source(expr, sw.nparams);  // a rejected expression: before any device call
  MIINT_CHECK(device_count() >= 1, who + " need a HIP device (no HIP devices visible)");
  set_device(0);
  ExprAdaptiveSweep es(expr, sw.nparams, 0);
  const AdaptSweepResult r = ranged ? es.integrate_ranges(sw.params, sw.rows, lo, hi, o)
                                    : es.integrate(sw.params, sw.rows, cfg.a, cfg.b, o);
  const double secs = wall_seconds() - process_start_seconds();
  uint64_t missed = 0;
  for (uint8_t c : r.converged) missed += c ? 0 : 1;
  if (missed)
    std::fprintf(stderr, "riemann: not converged: %llu of %llu rows (see converged, capped, "
                 "nonfinite and forced per row with --json)\n",
                 static_cast<unsigned long long>(missed),
                 static_cast<unsigned long long>(sw.rows));
  if (!a.flag("json"))
    for (uint64_t k = 0; k < sw.rows; ++k) {
      std::printf("%llu", static_cast<unsigned long long>(k));
      for (int j = 0; j < sw.nparams; ++j) std::printf(" %.17g", sw.params[k * sw.nparams + j]);
      std::printf(" %.17g\n", r.value[k]);
    }
  const std::string bits = json_bits(r.value);
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr);
  if (ranged) rec.add_raw("a", json_doubles(lo)).add_raw("b", json_doubles(hi));
  else rec.add("a", cfg.a).add("b", cfg.b);
  rec.add("rows", static_cast<double>(sw.rows)).add("nparams", sw.nparams)
      .add("rtol", used.rtol).add("atol", used.atol)
      .add("panels", static_cast<double>(used.panels)).add("max_depth", used.max_depth)
      .add("max_intervals", static_cast<double>(used.max_intervals))
      .add("max_total", static_cast<double>(used.max_total))
      .add_raw("value", json_doubles(r.value)).add_raw("value_bits", bits)
      .add_raw("err_est", json_doubles(r.err_est)).add_raw("resabs", json_doubles(r.resabs))
      .add_raw("tol", json_doubles(r.tol)).add_raw("converged", json_flags(r.converged))
      .add_raw("evals", json_counts(r.evals)).add_raw("rounds", json_counts(r.rounds))
      .add_raw("intervals", json_counts(r.intervals)).add_raw("splits", json_counts(r.splits))
      .add_raw("floor", json_counts(r.floor)).add_raw("forced", json_counts(r.forced))
      .add_raw("nonfinite", json_counts(r.nonfinite)).add_raw("capped", json_flags(r.capped))
      .add("not_converged", static_cast<double>(missed))
      .add("call_rounds", static_cast<double>(r.call_rounds))
      .add("call_evals", static_cast<double>(r.call_evals))
      .add("peak", static_cast<double>(r.peak)).add("range", r.range);
  cli::emit(a, rec.add("device_ms", r.device_ms).add("seconds_wall", secs));
  return 0;
}


// --expr with --curve-rtol / --curve-atol: the running integral F(x_j) from x_0 on a grid, every
// cell to a tolerance (ExprAdaptiveCurve). The grid is --a A --b B --points M (M equal cells) or
// --at FILE (one point per line). One GPU, one rank. Refusals come before any device call.
bool curve_requested(const cli::Args& a) {
  return a.has("curve-rtol") || a.has("curve-atol") || a.has("points") || a.has("at");
}

int run_expr_curve(const cli::Args& a) {
  const std::string who = "--curve-rtol / --curve-atol";
  MIINT_CHECK(a.has("curve-rtol") || a.has("curve-atol"),
              "--points / --at are the grid of a running integral to a tolerance: they need " +
                  who);
  MIINT_CHECK(a.has("expr"), who + " are the tolerance of an --expr running integral");
  for (const char* k : {"n", "rule", "running", "every", "running-out", "rtol", "atol",
                        "row-rtol", "row-atol", "ranges", "area-rtol", "area-atol", "panels-y",
                        "y-lo", "y-hi", "ya", "yb", "ny", "box", "osc", "omega", "max-cycles",
                        "params", "linspace", "loopback", "m", "shifts", "seed", "z", "periodic",
                        "m-max"})
    MIINT_CHECK(!a.has(k), who + " are the tolerance of a running integral on a grid: --" + k +
                               " does not go with them");
  MIINT_CHECK(a.integer("gpus", 1) <= 1, who + " run on one GPU: --gpus " + a.str("gpus", "") +
                                             " does not go with them");
  MIINT_CHECK(cli::env_int("WORLD_SIZE", 1) <= 1,
              who + " run as one rank: a rank environment (WORLD_SIZE = " +
                  std::to_string(cli::env_int("WORLD_SIZE", 1)) + ") does not go with them");
  MIINT_CHECK(!cli::on_cpu(a), who + " have no host engine: --device cpu does not go with them");
  std::vector<double> x;
  if (a.has("at")) {
    MIINT_CHECK(!(a.has("a") || a.has("b") || a.has("points")),
                "--at FILE is the whole grid: --a / --b / --points do not go with it");
    x = load_columns(a.str("at", ""), 1, "--at", "x");
  } else {
    MIINT_CHECK(a.has("a") && a.has("b") && a.has("points"),
                who + " need a grid: --a A --b B --points M, or --at FILE");
    const double lo = a.num("a", 0.0), hi = a.num("b", 0.0);
    MIINT_CHECK(!std::isinf(lo) && !std::isinf(hi),
                who + " take a finite grid: --a " + a.str("a", "") + " --b " + a.str("b", "") +
                    " has an infinite end");
    const double cells = adaptive_number(a, "points", 0.0, true);
    MIINT_CHECK(cells >= 1 && cells <= static_cast<double>(kAdaptCurveMaxCells),
                "--points " + a.str("points", "") + " must be 1..2^20");
    const uint64_t m = static_cast<uint64_t>(cells);
    // x_j = a + ((b - a) j) / M, the last one b: the adaptive rules' edges
    for (uint64_t j = 0; j <= m; ++j)
      x.push_back(j == m ? hi : lo + ((hi - lo) * static_cast<double>(j)) / cells);
  }
  AdaptSweepOptions o;
  o.rtol = adaptive_number(a, "curve-rtol", o.rtol, false);
  o.atol = adaptive_number(a, "curve-atol", 0.0, false);
  const double panels = adaptive_number(a, "panels", 0.0, true);
  const double depth = adaptive_number(a, "max-depth", o.max_depth, true);
  const double max_iv = adaptive_number(a, "max-intervals", 0.0, true);
  const double max_total = adaptive_number(a, "max-total", static_cast<double>(o.max_total), true);
  MIINT_CHECK(panels >= 0 && max_iv >= 0 && max_total >= 0 && std::fabs(depth) < 1e9,
              "--panels, --max-intervals, --max-total and --max-depth must not be negative or "
              "huge");
  o.panels = static_cast<uint64_t>(panels);
  o.max_depth = static_cast<int>(depth);
  o.max_intervals = static_cast<uint64_t>(max_iv);
  o.max_total = static_cast<uint64_t>(max_total);
  const AdaptSweepOptions used = adapt_curve_check(x, o);
  const std::string expr = a.str("expr", "");
  (void)expr_adapt_sweep_source(expr, 0);  // a rejected expression: before any device call
  MIINT_CHECK(device_count() >= 1, who + " need a HIP device (no HIP devices visible)");
  set_device(0);
  ExprAdaptiveCurve ec(expr, 0);
  const AdaptCurveResult r = ec.integrate(x, o);
  const double secs = wall_seconds() - process_start_seconds();
  if (r.unconverged) {
    uint64_t first = 0;
    while (first < r.cells.rows() && r.cells.converged[first]) ++first;
    std::fprintf(stderr, "riemann: not converged: %llu of %llu cells, the first one cell %llu "
                 "(see converged per point and capped, nonfinite and forced per cell with "
                 "--json)\n", static_cast<unsigned long long>(r.unconverged),
                 static_cast<unsigned long long>(r.cells.rows()),
                 static_cast<unsigned long long>(first));
  }
  if (!a.flag("json"))
    for (uint64_t j = 0; j < r.points(); ++j)
      std::printf("%.17g %.17g %.3g\n", r.x[j], r.value[j], r.err_est[j]);
  const AdaptSweepResult& c = r.cells;
  cli::JsonRecord cells;
  cells.add_raw("value", json_doubles(c.value)).add_raw("err_est", json_doubles(c.err_est))
      .add_raw("resabs", json_doubles(c.resabs)).add_raw("tol", json_doubles(c.tol))
      .add_raw("converged", json_flags(c.converged)).add_raw("evals", json_counts(c.evals))
      .add_raw("rounds", json_counts(c.rounds)).add_raw("intervals", json_counts(c.intervals))
      .add_raw("splits", json_counts(c.splits)).add_raw("floor", json_counts(c.floor))
      .add_raw("forced", json_counts(c.forced)).add_raw("nonfinite", json_counts(c.nonfinite))
      .add_raw("capped", json_flags(c.capped));
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr)
      .add("points", static_cast<double>(r.points())).add("rtol", used.rtol)
      .add("atol", used.atol).add("panels", static_cast<double>(used.panels))
      .add("max_depth", used.max_depth)
      .add("max_intervals", static_cast<double>(used.max_intervals))
      .add("max_total", static_cast<double>(used.max_total))
      .add_raw("x", json_doubles(r.x)).add_raw("value", json_doubles(r.value))
      .add_raw("value_bits", json_bits(r.value)).add_raw("err_est", json_doubles(r.err_est))
      .add_raw("tol", json_doubles(r.tol)).add_raw("resabs", json_doubles(r.resabs))
      .add_raw("converged", json_flags(r.converged))
      .add_raw("atol_cell", json_doubles(r.atol_cell)).add_raw("cells", cells.str())
      .add("total", r.total).add("not_converged", static_cast<double>(r.unconverged))
      .add("call_rounds", static_cast<double>(r.call_rounds))
      .add("call_evals", static_cast<double>(r.call_evals))
      .add("peak", static_cast<double>(r.peak));
  cli::emit(a, rec.add("device_ms", r.device_ms).add("seconds_wall", secs));
  return 0;
}

// --expr with --box A0:B0,A1:B1,...: the integral of f(x0, ..., x{d-1}) over the box by a
// randomly shifted rank-1 lattice rule (ExprLattice). --m M: the rule of n = 2^M points; --rtol R
// and / or --atol T instead: the walk of M from 12 to --m-max. Ranks split the points. A number
// that does not parse, or a flag of another mode, is refused before any device call.
std::vector<std::string> split_commas(const std::string& text) {
  std::vector<std::string> out(1);
  for (char c : text) {
    if (c == ',') out.emplace_back();
    else out.back() += c;
  }
  return out;
}

LatticeBox parse_box(const std::string& text) {
  LatticeBox box;
  for (const std::string& side : split_commas(text)) {
    const char* s = side.c_str();
    char* end = nullptr;
    const double lo = std::strtod(s, &end);
    MIINT_CHECK(end != s && *end == ':', "--box wants A0:B0,A1:B1,... (got '" + text + "')");
    const char* t = end + 1;
    const double hi = std::strtod(t, &end);
    MIINT_CHECK(end != t && *end == '\0', "--box wants A0:B0,A1:B1,... (got '" + text + "')");
    box.emplace_back(lo, hi);
  }
  return box;
}

int run_expr_lattice(const cli::Args& a, int iters) {
  for (const char* k : {"a", "b", "n", "rule", "running", "ya", "yb", "ny", "params", "linspace",
                        "every", "running-out", "panels", "max-depth", "max-intervals"})
    MIINT_CHECK(!a.has(k), std::string("--box integrates over a box by a lattice rule: --") + k +
                               " does not go with it");
  MIINT_CHECK(!cli::on_cpu(a), "--box has no host engine: --device cpu does not go with it");
  const bool walk = a.has("rtol") || a.has("atol");
  MIINT_CHECK(walk != a.has("m"), "--box takes --m M (the rule of 2^M points) or --rtol R / "
                                  "--atol T (the walk over M), one of the two");
  MIINT_CHECK(walk || !a.has("m-max"), "--m-max belongs to --box with --rtol / --atol");
  MIINT_CHECK(!walk || !a.has("z"), "--z is the generating vector of one --m, not of a walk");
  const LatticeBox box = parse_box(a.str("box", ""));
  const int d = static_cast<int>(box.size());
  LatticeOptions o;
  o.shifts = static_cast<int>(adaptive_number(a, "shifts", o.shifts, true));
  const double seed = adaptive_number(a, "seed", 0.0, true);
  MIINT_CHECK(seed >= 0, "--seed must not be negative");
  o.seed = static_cast<uint64_t>(seed);
  o.rtol = adaptive_number(a, "rtol", 0.0, false);
  o.atol = adaptive_number(a, "atol", 0.0, false);
  o.m_max = static_cast<int>(adaptive_number(a, "m-max", 0.0, true));
  MIINT_CHECK(!a.has("m-max") || o.m_max >= 1, "--m-max must be >= 1");
  const int m = static_cast<int>(adaptive_number(a, "m", 0.0, true));
  if (a.has("z"))
    for (const std::string& t : split_commas(a.str("z", ""))) {
      char* end = nullptr;
      const unsigned long long v = std::strtoull(t.c_str(), &end, 10);
      MIINT_CHECK(end != t.c_str() && *end == '\0' && t[0] != '-',
                  "--z wants odd whole numbers Z0,Z1,... (got '" + a.str("z", "") + "')");
      o.z.push_back(v);
    }
  const bool periodic = a.flag("periodic");
  const bool empty = std::any_of(box.begin(), box.end(), [](const std::pair<double, double>& p) {
    return p.first == p.second;
  });
  if (walk) lattice_check_walk(box, o);
  else lattice_check(box, m, o, 0, m >= kLatticeMinM && m <= kLatticeMaxM ? 1ull << m : 0);
  const std::string expr = a.str("expr", "");
  // a rejected expression, or an xJ the box has no side for: before any device call
  (void)expr_lattice_compile(expr, d, periodic);
  const cli::Topology topo = cli::topology(a);
  LatticeResult res;
  double dev_ms = 0.0;
  std::mutex mu;
  cli::RankFacts facts;
  cli::run_ranks(topo, [&](int rank, int dev, const Comm* comm) {
    ExprLattice el(expr, d, periodic, dev, 0);
    RankAgree agree(comm);
    LatticeResult r;
    double ms = 0.0;
    if (walk) {
      r = el.integrate_to(box, o, 1.0, comm);
      ms = agree.max(r.device_ms);
    } else {
      uint64_t b = 0, c = 0;
      rank_slice(1ull << m, rank, topo.world, &b, &c);
      r = el.integrate(box, m, o, b, c, 1.0, comm);
      r.evals = static_cast<uint64_t>(r.shifts) << m;  // the whole rule's, over all ranks
      // barrier right before the clock starts; the slowest rank's time
      ms = empty ? 0.0  // a side of no width: nothing was launched
                   : agree.max(el.time(box, m, o, b, c, iters, [&] { agree.barrier(); },
                                     [&] { fault::delay(rank); }));
    }
    std::lock_guard<std::mutex> g(mu);
    if (rank == topo.rank0) {
      res = r;
      dev_ms = ms;
      facts.note(comm);
    }
  });
  if (topo.rank0 != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  if (walk && !res.converged)
    std::fprintf(stderr, "riemann: not converged: err_est %.3g after %d levels (m = %d)\n",
                 res.err_est, res.levels, res.m);
  if (!a.flag("json")) std::printf("%.17g +- %.3g\n", res.value, res.err_est);
  std::string bs = "[", es = "[";
  for (size_t j = 0; j < box.size(); ++j) {
    char b[80];
    std::snprintf(b, sizeof b, "%s[%.17g,%.17g]", j ? "," : "", box[j].first, box[j].second);
    bs += b;
  }
  for (size_t k = 0; k < res.estimates.size(); ++k) {
    char b[40];
    if (std::isfinite(res.estimates[k]))
      std::snprintf(b, sizeof b, "%s%.17g", k ? "," : "", res.estimates[k]);
    else
      std::snprintf(b, sizeof b, "%snull", k ? "," : "");
    es += b;
  }
  cli::JsonRecord rec;
  rec.add("program", "riemann").add("expr", expr).add_raw("box", bs + "]").add("d", d)
      .add("m", res.m).add("n", static_cast<double>(res.n)).add("shifts", res.shifts)
      .add("seed", static_cast<double>(o.seed)).add("periodic", periodic)
      .add("gpus", topo.world).add("value", res.value).add("err_est", res.err_est)
      .add_raw("estimates", es + "]").add("evals", static_cast<double>(res.evals))
      .add("levels", res.levels).add("converged", res.converged);
  if (walk) rec.add("rtol", o.rtol).add("atol", o.atol);
  char bits[24];
  uint64_t w = 0;
  std::memcpy(&w, &res.value, sizeof w);
  std::snprintf(bits, sizeof bits, "%016llx", static_cast<unsigned long long>(w));
  rec.add("value_bits", bits);
  std::memcpy(&w, &res.err_est, sizeof w);
  std::snprintf(bits, sizeof bits, "%016llx", static_cast<unsigned long long>(w));
  rec.add("err_est_bits", bits);
  facts.add(rec, topo);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    rec.add("analytic", exact).add("abs_err", std::fabs(res.value - exact));
  }
  cli::emit(a, rec.add("device_ms", dev_ms)
                   .add("samples_per_s",
                        dev_ms > 0 ? static_cast<double>(res.evals) / (dev_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

// --expr (see the header comment): GPU ranks as in the default path, f compiled by hipRTC.
int run_expr(const cli::Args& a, const RiemannConfig& cfg, double nd, int iters) {
  if (area_adaptive_requested(a)) return run_expr_adaptive2d(a, cfg);
  if (row_adaptive_requested(a)) return run_expr_adaptive_sweep(a, cfg);
  if (a.has("box")) return run_expr_lattice(a, iters);
  if (adaptive_requested(a)) return run_expr_adaptive(a, cfg);
  if (a.has("ya")) return run_expr2d(a, cfg, nd, iters);
  if (a.flag("running")) return run_expr_running(a, cfg, nd);
  if (a.has("params") || a.has("linspace")) return run_expr_sweep(a, cfg, nd, iters);
  if (cli::on_cpu(a)) return run_host_expr(a, cfg, nd, iters);
  const std::string expr = a.str("expr", "");
  const cli::Topology topo = cli::topology(a);
  double result = 0.0, dev_ms = 0.0;
  std::mutex mu;
  cli::RankFacts facts;
  cli::run_ranks(topo, [&](int rank, int dev, const Comm* comm) {
    ExprIntegrator ei(expr, dev);
    RankAgree agree(comm);
    uint64_t b = 0, c = 0;
    rank_slice(cfg.n, rank, topo.world, &b, &c);
    const double v = ei.integrate(cfg.a, cfg.b, cfg.n, cfg.rule, b, c, 1.0, comm);
    // barrier right before the clock starts; the slowest rank's time
    const double ms = agree.max(ei.time(cfg.a, cfg.b, cfg.n, cfg.rule, b, c, iters,
                                        [&] { agree.barrier(); }, [&] { fault::delay(rank); }));
    std::lock_guard<std::mutex> g(mu);
    if (rank == topo.rank0) {
      result = v;
      dev_ms = ms;
      facts.note(comm);
    }
  });
  if (topo.rank0 != 0) return 0;
  const double secs = wall_seconds() - process_start_seconds();
  print_result(secs, cfg.b, nd, result);
  cli::JsonRecord r;
  r.add("program", "riemann")
      .add("expr", expr)
      .add("a", cfg.a)
      .add("b", cfg.b)
      .add("n", nd)
      .add("rule", a.str("rule", "left"))
      .add("gpus", topo.world)
      .add("result", result);
  facts.add(r, topo);
  if (a.has("analytic")) {
    const double exact = a.num("analytic", 0.0);
    r.add("analytic", exact).add("abs_err", std::fabs(result - exact));
  }
  cli::emit(a, r.add("device_ms", dev_ms)
                   .add("subintervals_per_s", dev_ms > 0 ? nd / (dev_ms * 1e-3) : 0.0)
                   .add("seconds_wall", secs));
  return 0;
}

}  // namespace

constexpr const char* kUsage =
    "usage: riemann [--n 1e9] [--gpus G] [--loopback W] [--integrand sin|pi4|poly|train|table]\n"
    "               [--rule left|mid|right] [--dtype fp64|fp32|fp32acc] [--div series_exact|series|ieee]\n"
    "               [--iters K] [--block 64..1024] [--grid G] [--a A --b B] [--parity]\n"
    "               [--one-shot | --no-one-shot] [--no-multistep] [--unfused]\n"
    "               [--json] [--jsonl FILE] [--profile FILE]\n"
    "               [--device cpu [--threads T] [--ranks P]]\n"
    "               [--expr EXPR --a A --b B [--analytic V]]\n"
    "               [--expr EXPR --params FILE | --linspace p0=LO:HI:COUNT]\n"
    "               [--expr EXPR --a A --b B --n N --running [--every K] [--running-out FILE]]\n"
    "               [--expr EXPR --a AX --b BX --ya AY --yb BY [--n NX] [--ny NY] [--analytic V]]\n"
    "               [--expr EXPR --a AX --b BX --ya AY --yb BY --area-rtol R [--area-atol T]\n"
    "                [--panels P] [--panels-y Q] [--max-depth D] [--max-intervals M]]\n"
    "               [--expr EXPR --a AX --b BX --y-lo EXPR --y-hi EXPR --area-rtol R [--area-atol T]\n"
    "                [--panels P] [--panels-y Q] [--max-depth D] [--max-intervals M]]\n"
    "               [--expr EXPR --a A --b B --rtol R [--atol T] [--panels P] [--max-depth D]\n"
    "                [--max-intervals M]]\n"
    "               [--expr EXPR --a A --b B|inf --osc cos|sin --omega W --rtol R [--atol T]\n"
    "                [--panels P] [--max-depth D] [--max-intervals M] [--max-cycles C]]\n"
    "               [--expr EXPR --a A --b B --params FILE | --linspace p0=LO:HI:COUNT --row-rtol R\n"
    "                [--row-atol T] [--panels P] [--max-depth D] [--max-intervals M] [--max-total N]]\n"
    "               [--expr EXPR --ranges FILE --params FILE | --linspace p0=LO:HI:COUNT --row-rtol R\n"
    "                [--row-atol T] [--panels P] [--max-depth D] [--max-intervals M] [--max-total N]]\n"
    "               [--expr EXPR --a A --b B --points M | --at FILE --curve-rtol R [--curve-atol T]\n"
    "                [--panels P] [--max-depth D] [--max-intervals M] [--max-total N]]\n"
    "               [--expr EXPR --box A0:B0,A1:B1,... --m M | --rtol R [--atol T] [--m-max M]\n"
    "                [--shifts R] [--seed S] [--periodic] [--z Z0,Z1,...] [--analytic V]]\n"
    "Riemann sum of f on [a, b] (default sin on [0, pi], N = 1e9); prints the reference's\n"
    "two lines, or one JSON record with --json. Multi-GPU: --gpus G, torchrun or miintrun.\n"
    "--running: the running integral F(x) = h * sum of f up to x at every sample (one GPU,\n"
    "  one rank): every K-th value with --every K (global sample index: (i + 1) % K == 0);\n"
    "  values go to --running-out FILE as raw little-endian fp64, else to stdout as 'x value'\n"
    "  lines, refused above 10000 lines; --json adds total, outputs, every and device_ms.\n"
    "--ya AY --yb BY: the double integral of --expr over x and y on [AX, BX] x [AY, BY], NX x NY\n"
    "  samples (--ny defaults to --n), the same rule on both axes; ranks split the sample rows\n"
    "  (--gpus, --loopback, rank environment, --device cpu [--threads T] as for --expr);\n"
    "  --json: expr, a, b, ya, yb, n, ny, rule, value, device_ms, samples_per_s.\n"
    "--area-rtol R / --area-atol T: with --ya AY --yb BY, the double integral of --expr over the\n"
    "  finite rectangle to the tolerance max(T, R |value|): the (7, 15) x (7, 15) Gauss-Kronrod\n"
    "  product, 225 evaluations a rectangle, from --panels P x --panels-y Q equal rectangles\n"
    "  (default 64, Q defaults to P), each bisected along the axis with the larger error, at most\n"
    "  --max-depth D times per axis (default 60), at most --max-intervals M rectangles in all\n"
    "  (default 2^22). Prints the value, and a warning on stderr when not converged; --json:\n"
    "  value, err_est, resabs, tol, converged, evals, rounds, intervals, splits, splits_x,\n"
    "  splits_y, floor, forced, nonfinite, capped, device_ms. One GPU, one rank, no host engine:\n"
    "  refused without --ya / --yb, with --n, --ny, --rule, --running, --params, --linspace, --box,\n"
    "  --rtol, --atol, --row-rtol, --row-atol, --gpus above 1, --loopback, WORLD_SIZE above 1 or\n"
    "  --device cpu, and with an infinite side. A discontinuity along a curve (an indicator) runs\n"
    "  to the cap and reports capped: use --y-lo / --y-hi, the fixed rule or --box there.\n"
    "--y-lo EXPR --y-hi EXPR: with --area-rtol R / --area-atol T and in place of --ya / --yb, the\n"
    "  double integral of --expr over AX <= x <= BX, y_lo(x) <= y <= y_hi(x), both limits\n"
    "  expressions over x alone (write --y-lo=-sqrt(1.0-x*x) where one begins with a minus). The\n"
    "  region is mapped onto [AX, BX] x [0, 1] by y = y_lo + (y_hi - y_lo) v and the rounds above\n"
    "  run on f (y_hi - y_lo): err_est, resabs and tol are the mapped integrand's, --panels-y\n"
    "  divides v. Where y_hi(x) < y_lo(x) the strip counts negatively; a limit that is not finite\n"
    "  at a node counts as nonfinite. The outputs are those of the rectangle form (ya 0, yb 1);\n"
    "  --json adds y_lo, y_hi. Refused with one limit alone, without --area-rtol / --area-atol,\n"
    "  with --ya / --yb, with a y in a limit and with whatever --area-rtol refuses.\n"
    "--rtol R / --atol T: the integral of --expr on [A, B] to the tolerance max(T, R |value|)\n"
    "  (adaptive Gauss-Kronrod (7, 15) from --panels P equal intervals, default 65536, bisected at\n"
    "  most --max-depth D times, default 60, at most --max-intervals M in all, default 2^22);\n"
    "  prints the value, and a warning on stderr when not converged; --json: value, err_est,\n"
    "  resabs, tol, converged, evals, rounds, intervals, splits, floor, forced, nonfinite, capped,\n"
    "  device_ms. One GPU, one rank, no host engine: refused with --n, --rule, --running, --ya,\n"
    "  --params, --linspace, --gpus above 1, --loopback, WORLD_SIZE above 1 or --device cpu.\n"
    "  A and B may be inf, +inf, -inf or infinity (any case): (A, inf), (-inf, B) and (-inf, inf)\n"
    "  are mapped onto t in (0, 1] by x = A + (1 - t) / t, x = B - (1 - t) / t, or both halves at\n"
    "  once, and the rounds bisect t; --json adds range: finite, upper, lower or both. There\n"
    "  resabs is the integral of |f(x) + f(-x)| over (0, inf) for (-inf, inf). A singularity at the\n"
    "  finite end (exp(-x)/sqrt(x) on (0, inf)) ends as nonfinite: split it at 1; an oscillatory\n"
    "  tail (sin(x)/x) does not converge, and the run says so. The same holds with --row-rtol.\n"
    "  An infinite A or B without --rtol / --atol / --row-rtol / --row-atol is refused.\n"
    "--osc cos|sin --omega W: with --rtol R / --atol T, the integral of --expr times cos(W x) or\n"
    "  sin(W x) on [A, B] to the tolerance, at a cost that does not grow with W: adaptive\n"
    "  Filon-Clenshaw-Curtis (13, 25), 25 evaluations an interval, the weight integrated exactly;\n"
    "  --panels, --max-depth and --max-intervals as for --rtol. f must be finite on the closed\n"
    "  range (both ends of every interval are evaluated). --b inf is the Fourier tail on (A, inf):\n"
    "  W != 0 and --atol are required (--rtol alone is refused), --panels is per cycle (default\n"
    "  16), --max-cycles C bounds it (default 50). --json adds omega, kind, cycles, extrapolated,\n"
    "  reason. Refused, naming the conflict: --osc without --omega and the reverse, no tolerance,\n"
    "  --n, --rule, --running, --ya, --y-lo, --box, --params, --linspace, --row-rtol, --area-rtol,\n"
    "  --gpus above 1, --loopback, WORLD_SIZE above 1, --device cpu, --a -inf.\n"
    "--row-rtol R / --row-atol T: with --params or --linspace, the integral of --expr on [A, B] for\n"
    "  every row to the row's own tolerance max(T, R |value of the row|), the rows sharing the\n"
    "  rounds (--panels P per row, default: 65536 / rows as a power of two, at least 16;\n"
    "  --max-intervals M per row, default --max-total / rows; --max-total N for all rows together,\n"
    "  default 2^22; --max-depth D). Prints 'row parameters value' lines and one warning on stderr\n"
    "  with the number of rows not converged; --json: the per-row arrays value, value_bits, err_est,\n"
    "  resabs, tol, converged, evals, rounds, intervals, splits, floor, forced, nonfinite, capped,\n"
    "  and rows, call_rounds, call_evals, peak, device_ms. Refused with --rtol, --atol, --n, --rule,\n"
    "  --running, --ya, --box, --gpus above 1, --loopback, WORLD_SIZE above 1 or --device cpu.\n"
    "  --ranges FILE (K lines 'a b') in place of --a / --b: row r on its own finite [a_r, b_r],\n"
    "  bitwise what the one-row call on that range gives; a_r > b_r negates the row, a_r == b_r\n"
    "  gives 0. Refused with --a / --b, without a row tolerance, and with an infinite end.\n"
    "--curve-rtol R / --curve-atol T: the running integral F(x_j) of --expr from x_0 at the points\n"
    "  of a grid, --a A --b B --points M (M equal cells) or --at FILE (one point per line, strictly\n"
    "  increasing or strictly decreasing): every cell to max(T |cell| / |grid|, R |its integral|),\n"
    "  so err_est at a point is held to at most T + R * (the integral of |f| up to it). --panels P\n"
    "  and --max-intervals M are per cell (default: 65536 / cells as a power of two, at least 1;\n"
    "  --max-total / cells); --max-total N, --max-depth D. Prints 'x F err_est' lines and one\n"
    "  warning on stderr if a cell did not converge; --json: the per-point arrays x, value,\n"
    "  value_bits, err_est, tol, resabs, converged, the per-cell arrays in cells, atol_cell, total,\n"
    "  call_rounds, call_evals, peak, device_ms. Refused with --n, --rule, --running, --rtol,\n"
    "  --row-rtol, --area-rtol, --ya, --box, --osc, --params, --gpus above 1, --loopback,\n"
    "  WORLD_SIZE above 1, --device cpu, an infinite end, --at with --a / --b / --points.\n"
    "--box A0:B0,A1:B1,...: the integral of --expr over x0, x1, ... (at most 16 sides) by a randomly\n"
    "  shifted rank-1 lattice rule: --m M for n = 2^M points (built-in generating vectors for M =\n"
    "  10..26, else --z Z0,Z1,... odd and below n), --shifts R random shifts (default 16) from\n"
    "  --seed S, the tent transform unless --periodic; or --rtol R / --atol T (here the lattice's\n"
    "  tolerance): M walks from 12 to --m-max until err_est <= max(T, R |value|). Prints 'value +-\n"
    "  err_est' (one standard error over the shifts); --json: value, err_est, estimates, m, n,\n"
    "  shifts, evals, levels, converged, device_ms. Ranks split the points (--gpus, --loopback,\n"
    "  rank environment). Refused with --a, --b, --n, --rule, --running, --ya, --params,\n"
    "  --linspace, --panels, --max-depth, --max-intervals or --device cpu.\n";

int main(int argc, char** argv) {
  try {
    install_crash_handler_from_env();
    cli::Args a(argc, argv);
    if (cli::usage_requested(a, kUsage)) return 0;
    if (curve_requested(a)) return run_expr_curve(a);  // it names its own conflicts
    MIINT_CHECK(row_adaptive_requested(a) || !a.has("ranges"),
                "--ranges gives the rows of a sweep to a tolerance their own ranges: it needs "
                "--row-rtol R / --row-atol T");
    const Integrand f = cli::parse_integrand(a.str("integrand", "sin"));
    const double pi = 3.14159265358979323846;
    double lo = 0.0, hi = pi;  // riemann.cpp:6 RANGE = M_PI
    if (f == Integrand::kPi4) hi = 1.0;
    std::vector<double> prof;  // table integrand: --profile FILE or the built-in profile
    if (f == Integrand::kTable)
      prof = a.has("profile") ? oracle::load_profile(a.str("profile", "")) : oracle::profile_table();
    if (f == Integrand::kTrainVel) hi = 1800.0;
    if (f == Integrand::kTable) hi = static_cast<double>(prof.size() - 1);
    lo = a.num("a", lo);
    hi = a.num("b", hi);
    MIINT_CHECK((std::isfinite(lo) && std::isfinite(hi)) || std::isnan(lo) || std::isnan(hi) ||
                    (a.has("expr") && (adaptive_requested(a) || row_adaptive_requested(a))),
                "--a " + a.str("a", "") + " --b " + a.str("b", "") + ": an infinite range needs "
                "--expr with --rtol / --atol or --row-rtol / --row-atol (the fixed rules have no "
                "such range)");
    const double nd = a.num("n", 1e9);  // riemann.cpp:10 STEPS
    const auto n = static_cast<uint64_t>(nd);
    const int iters = static_cast<int>(a.integer("iters", 1));
    MIINT_CHECK(iters >= 1, "--iters must be >= 1");

    RiemannConfig cfg;
    cfg.integrand = f;
    cfg.a = lo;
    cfg.b = hi;
    cfg.n = n;
    cfg.rule = cli::parse_rule(a.str("rule", "left"));
    cfg.dtype = cli::parse_dtype(a.str("dtype", "fp64"));
    cfg.div = cli::parse_div(a.str("div", "series_exact"));
    cfg.fused = !a.flag("unfused");
    cfg.multistep = !a.flag("no-multistep");  // chained batches, full auto grid
    // --block: threads per workgroup (the reference's SP, cintegrate.cu:17-18); --grid:
    // workgroups (its SM), 0 = auto
    cfg.block = static_cast<int>(a.integer("block", kRiemannBlock));
    cfg.grid = static_cast<int>(a.integer("grid", 0));
    MIINT_CHECK(riemann_block_ok(cfg.block), "--block must be 64, 128, 256, 512 or 1024");
    if (f == Integrand::kTrainVel) { cfg.p0 = oracle::kTrainTs; cfg.p1 = oracle::kTrainVs; }
    if (f == Integrand::kTable) cfg.table = prof;
    if (f == Integrand::kPoly) cfg.coef = {1.0, -0.5, 0.25, 0.125};

    if (osc_requested(a)) return run_expr_osc(a, cfg);  // it names its own conflicts
    MIINT_CHECK(a.has("expr") || !(a.has("params") || a.has("linspace")),
                "--params / --linspace sweep the parameters of an --expr integrand");
    MIINT_CHECK(a.has("expr") || !a.has("running"),
                "--running is the running integral of an --expr integrand");
    MIINT_CHECK(a.flag("running") || !(a.has("every") || a.has("running-out")),
                "--every / --running-out belong to --running");
    MIINT_CHECK(!region_requested(a) || !(a.has("ya") || a.has("yb")),
                "--y-lo / --y-hi are the limits in y as expressions over x: --ya / --yb (the "
                "limits as numbers) do not go with them");
    MIINT_CHECK(a.has("ya") == a.has("yb"),
                "--ya and --yb go together: the y interval of a double integral");
    MIINT_CHECK(a.has("ya") || region_requested(a) || !a.has("ny"),
                "--ny belongs to a double integral (--ya AY --yb BY)");
    MIINT_CHECK(a.has("expr") || !a.has("ya"),
                "--ya / --yb are the double integral of an --expr integrand over x and y");
    MIINT_CHECK(a.has("expr") || !adaptive_requested(a),
                "--rtol / --atol are the tolerance of an --expr integrand");
    MIINT_CHECK(a.has("expr") || !row_adaptive_requested(a),
                "--row-rtol / --row-atol are the per-row tolerance of an --expr parameter sweep");
    MIINT_CHECK(a.has("expr") || !area_adaptive_requested(a),
                "--area-rtol / --area-atol are the tolerance of an --expr double integral");
    MIINT_CHECK(a.has("expr") || !region_requested(a),
                "--y-lo / --y-hi are the limits in y of an --expr double integral");
    MIINT_CHECK(area_adaptive_requested(a) || !region_requested(a),
                "--y-lo / --y-hi are the limits of a double integral to a tolerance: they need "
                "--area-rtol R / --area-atol T (the fixed rule has no such region)");
    MIINT_CHECK(area_adaptive_requested(a) || !a.has("panels-y"),
                "--panels-y belongs to --area-rtol / --area-atol");
    MIINT_CHECK(adaptive_requested(a) || row_adaptive_requested(a) || area_adaptive_requested(a) ||
                    !(a.has("panels") || a.has("max-depth") || a.has("max-intervals")),
                "--panels / --max-depth / --max-intervals belong to --rtol / --atol");
    MIINT_CHECK(row_adaptive_requested(a) || !a.has("max-total"),
                "--max-total belongs to --row-rtol / --row-atol");
    MIINT_CHECK(a.has("expr") || !a.has("box"),
                "--box is the box of an --expr integrand over x0, x1, ...");
    for (const char* k : {"m", "shifts", "seed", "z", "periodic", "m-max"})
      MIINT_CHECK(a.has("box") || !a.has(k),
                  std::string("--") + k + " belongs to --box (the lattice rule of an --expr "
                  "integrand)");
    if (a.has("expr")) return run_expr(a, cfg, nd, iters);
    if (cli::on_cpu(a)) return run_host(a, cfg, nd, iters);
    const cli::Topology topo = cli::topology(a);

    double result = 0.0, dev_ms = 0.0, wall_ms = 0.0, one_shot_ms = 0.0;
    // The one-integration-per-call harness (~450 extra integrations) runs only for a record
    // (--json) or when asked (--one-shot): the default program is the reference's single run,
    // one cold + one timed integration before its "seconds" line (riemann.cpp:49-51,90-96)
    const bool one_shot = (a.flag("json") || a.flag("one-shot")) && !a.flag("no-one-shot");
    LaunchShape launch_shape{0, cfg.block};
    cli::RankFacts facts;
    std::mutex mu;
    std::vector<double> partials;  // --parity: the workers' partials, rank order
    if (a.flag("parity")) {
      // riemann.cpp:62-86 as a distributed program: P = world ranks -> W = P - 1 workers. Rank
      // 0 is the coordinator and integrates nothing; rank r >= 1 integrates worker r-1's
      // slice [(r-1) R/W, r R/W) with (int)(N / W) samples on its own GPU; the partials meet
      // in one allgather and rank 0 adds them in rank order (the MPI_Recv loop's rounding,
      // riemann.cpp:82-85). P = 1: no workers, the sum is 0 (B10).
      const int P = topo.world;
      const int W = P - 1;
      MIINT_CHECK(W < 1 || nd / W < 2147483648.0,
                  "--parity reproduces riemann.cpp's int local_n: N / (P - 1) must stay below 2^31");
      cli::run_ranks(topo, [&](int rank, int dev, const Comm* comm) {
        RankAgree agree(comm);
        std::unique_ptr<RiemannPlan> plan;
        if (rank >= 1) {
          RiemannConfig c = cfg;
          const int w = rank - 1;
          c.a = w * ((hi - lo) / W);
          c.b = c.a + (hi - lo) / W;
          c.n = static_cast<uint64_t>(static_cast<int>(nd / W));
          c.multistep = false;  // one integration: the full grid, one fused launch
          plan.reset(new RiemannPlan(c, dev));  // the worker's own; the partials meet below
          plan->run();                          // cold: code-object load, first launch
        }
        double partial = 0.0;
        std::vector<double> best;
        for (int it = 0; it < iters; ++it) {
          agree.barrier();
          const double t0 = wall_seconds();
          if (plan) partial = plan->run();
          const std::vector<double> all = agree.gather({partial});  // MPI_Send / MPI_Recv
          fault::delay(rank);
          best.push_back(agree.max((wall_seconds() - t0) * 1e3));
          if (rank == topo.rank0 && it + 1 == iters) {
            double g_sum = 0.0;
            for (int q = 1; q < P; ++q) g_sum += all[static_cast<size_t>(q)];  // rank order
            std::lock_guard<std::mutex> g(mu);
            result = g_sum;
            partials.assign(all.begin(), all.end());
          }
        }
        std::lock_guard<std::mutex> g(mu);
        if (rank == topo.rank0) {
          dev_ms = *std::min_element(best.begin(), best.end());
          wall_ms = dev_ms;
          facts.note(comm);
          if (plan) launch_shape = plan->shape();
        }
      });
    } else {
      cli::run_ranks(topo, [&](int rank, int dev, const Comm* comm) {
        RiemannPlan plan(cfg, dev, comm);
        RankAgree agree(comm);
        if (a.has("prepare")) plan.prepare_steps(static_cast<int>(a.integer("prepare", iters)));
        plan.run_steps(1, comm != nullptr, false);  // cold: code-object load, first launch
        // the timed steps: every rank's clock starts after a collective barrier, the time
        // reported is the slowest rank's (the reference's rank 0 stops its clock only after
        // every worker's result has arrived, riemann.cpp:82-93)
        StepTiming t = plan.run_steps(iters, comm != nullptr, iters > 1);
        const double ms = agree.max(t.device_ms / iters);
        const double wms = agree.max(t.wall_s * 1e3 / iters);
        const double v = plan.host_result(plan.host_index_of(iters - 1, iters > 1));
        // one integration per call, launch to pinned result (the reference's own timing unit)
        double shot = 0.0;
        if (one_shot) {
          if (!plan.collective()) {
            // 400 settling calls first: from idle the clocks take ~250 calls to settle. A
            // 1-step graph replay with the host polling the pinned result: the fastest form
            // (profiles/r4/one_shot_grid_settled.jsonl: 78.4-79 us against 80.1 direct_poll)
            try {
              shot = plan.time_one_shot(50, plan.direct() ? "graph_poll" : "direct", 400)
                         .median_us * 1e-3;
            } catch (const Error&) {
              // only a failed 1-step graph capture falls back to the direct launch; any other
              // failure (a replay whose value disagrees, a result never stored) propagates
              if (!plan.direct() || plan.graph_error().empty()) throw;
              shot = plan.time_one_shot(50, "direct_poll", 400).median_us * 1e-3;
            }
          } else {
            std::vector<double> v1;
            for (int k = 0; k < 10; ++k) v1.push_back(plan.run_steps(1, true, false).wall_s * 1e3);
            shot = agree.max(cli::median(v1));
          }
        }
        std::lock_guard<std::mutex> g(mu);
        if (rank == topo.rank0) {
          launch_shape = plan.shape();
          result = v;
          dev_ms = ms;
          wall_ms = wms;
          one_shot_ms = shot;
          facts.note(comm);
        }
      });
    }
    if (topo.rank0 != 0) return 0;
    const double secs = wall_seconds() - process_start_seconds();
    print_result(secs, hi, nd, result);
    const double exact = f == Integrand::kTable ? oracle::table_integral(prof, lo, hi)
                                                : oracle::analytic(f, lo, hi, cfg.coef, cfg.p0, cfg.p1);
    cli::JsonRecord rec;
    rec.add("program", "riemann")
        .add("integrand", a.str("integrand", "sin"))
        .add("dtype", a.str("dtype", "fp64"))
        .add("rule", a.str("rule", "left"))
        .add("n", nd)
        .add("gpus", topo.world)
        .add("parity", a.flag("parity"));
    facts.add(rec, topo);
    // --parity integrates W (int)(N / W) samples (fewer than N when W does not divide N)
    const int workers = topo.world - 1;
    const double work =
        !a.flag("parity") ? nd
                          : (workers >= 1 ? static_cast<double>(workers) *
                                                static_cast<int>(nd / workers)
                                          : 0.0);
    if (a.flag("parity")) {
      // the partials in rank order (rank 0, the coordinator, contributes 0)
      std::string ps = "[";
      for (size_t q = 0; q < partials.size(); ++q) {
        char b[40];
        std::snprintf(b, sizeof b, "%s%.17g", q ? "," : "", partials[q]);
        ps += b;
      }
      rec.add("workers", workers).add("samples", work).add_raw("partials", ps + "]");
    }
    rec.add("result", result)
        .add("analytic", exact)
        .add("abs_err", std::fabs(result - exact))
        .add("rel_err", std::fabs(result - exact) / std::fabs(exact))
        .add("block", launch_shape.block)
        .add("grid", launch_shape.grid)
        .add("device_ms", dev_ms)
        .add("seconds_device", dev_ms * 1e-3)
        .add("wall_ms_per_integration", wall_ms)
        .add("timing", a.flag("parity") ? "host, barrier to gathered partials, slowest rank"
                                        : "hipEvent per integration, slowest rank")
        .add("subintervals_per_s", dev_ms > 0 ? work / (dev_ms * 1e-3) : 0.0);
    rec.add("one_shot", one_shot && !a.flag("parity"));
    if (!a.flag("parity") && one_shot) rec.add("ms_one_shot", one_shot_ms);
    cli::emit(a, rec.add("seconds_wall", secs));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "riemann: %s\n", e.what());
    return 1;
  }
}
