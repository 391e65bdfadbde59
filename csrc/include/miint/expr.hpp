// Runtime integrands: f(x) given as an expression, compiled for gfx950 with hipRTC.
//
// The reference's integrand is hard-wired (riemann.cpp:37 `sin(x)`, cintegrate.cu:68) and
// changing it means editing the source and recompiling (no argv, no config).
// Here `riemann --expr "exp(-x*x)" --a 0 --b 3` (or kernels.riemann_expr in Python) turns
// the expression into a HIP device function `double f(double x) { return (EXPR); }`, builds a
// partial-sum kernel and a finalize kernel around it with hipRTC
// (--offload-arch=gfx950 -O3), loads the code object and integrates:
//
//   miint_expr_partials  2048 x 256 lanes, each a contiguous run of samples walked with an
//                        exact fp64 index, every sample evaluated in fp64 (4 accumulators),
//                        block reduction -> one partial per workgroup
//   miint_expr_finalize  the closing step -> h * scale * sum
//
// The block reduction (wave64 butterfly over __shfl_xor, then the four waves' sums through
// LDS) and the closing step (one workgroup sums the partials in index order, reduces and
// scales) are the same text in every family below: the device prelude of miint/expr_rtc.hpp,
// which also holds the compile cache, the module owner and the timing loop they share.
//
// Fixed grid and fixed reduction order: bitwise reproducible. Compiled programs are cached
// per (expression, device) in the process. The expression is one C++ expression over `x`
// using the HIP device math library (sin, exp, pow, ...): statements, braces, `asm` and
// string/char literals are rejected before anything is compiled.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "miint/comm.hpp"
#include "miint/common.hpp"
#include "miint/expr_rtc.hpp"
#include "miint/runtime.hpp"

namespace miint {

// Throws unless `expr` is one C++ expression over x (allowed characters only; no statements,
// braces, literals, asm/volatile/goto or __builtin_amdgcn*). Shared by the GPU and host JITs.
void expr_check(const std::string& expr);
// The kernel source generated for `expr` (throws on a rejected expression).
std::string expr_source(const std::string& expr);
// Compile `expr` for gfx950 with hipRTC (no device needed); returns the code object. Throws
// with the compiler log on failure.
std::string expr_compile(const std::string& expr);
namespace detail {
// hipRTC compile of `src` for gfx950 (-O3); `expr` names the expression in the error.
std::string rtc_compile(const std::string& src, const std::string& expr);
}  // namespace detail

class ExprIntegrator {
 public:
  ExprIntegrator(const std::string& expr, int device, int grid = 2048);
  ExprIntegrator(const ExprIntegrator&) = delete;
  ExprIntegrator& operator=(const ExprIntegrator&) = delete;
  // h * scale * sum f(a + (i + off) h) over samples [begin, begin + count) of an n-sample
  // rule on [a, b]; with a communicator the ranks' values are all-reduced (every rank gets
  // the global sum). Synchronous.
  double integrate(double a, double b, uint64_t n, Rule rule, uint64_t begin, uint64_t count,
                   double scale = 1.0, const Comm* comm = nullptr);
  // Device ms per integration over `iters` back-to-back integrations (events, no host sync
  // between them), for the same arguments. at_start runs on the host right before the first
  // event is recorded (a multi-rank caller's barrier), at_end right before the last one.
  double time(double a, double b, uint64_t n, Rule rule, uint64_t begin, uint64_t count,
              int iters, const std::function<void()>& at_start = {},
              const std::function<void()>& at_end = {});
  const std::string& expression() const { return expr_; }

 private:
  void check(uint64_t n, uint64_t begin, uint64_t count) const;
  void enqueue(double a, double h, double off, uint64_t begin, uint64_t count, double scale,
               hipStream_t s);
  std::string expr_;
  int device_, grid_;
  Stream stream_;
  DeviceBuffer<double> partials_, out_;
  PinnedBuffer<double> host_;
  Event e0_, e1_;
  detail::RtcModule module_;  // the last member: destroyed first (miint/expr_rtc.hpp)
};

// ---------------------------------------------------------------------------------------
// Parameter sweeps: f(x, p0, ..., p{nparams-1}) over K parameter rows in one launch.
//
// A family of integrals (exp(-p0*x*x) over 1000 widths) through ExprIntegrator costs a
// compile, a module load, two launches and a sync per value. Here the expression may also
// mention p0..p7; the rows' values are kernel data (params[k*nparams + j]), so one compile
// and one pair of launches serve every row:
//
//   miint_expr_sweep_partials  grid (gx, gy): gx sample slices x gy row lanes. Workgroup
//                              (bx, by) walks rows by, by + gy, ...; per row it runs the
//                              per-sample loop of miint_expr_partials over its bx share of
//                              the samples and writes one partial per (row, bx).
//   miint_expr_sweep_close     the closing step per row, over its gx partials
//                              -> out[k] = scale * sum
//
// Rows are independent and the close is its own kernel: no workgroup waits on another, so
// nothing depends on co-residency. gx depends on the sample count (and an explicit grid)
// only, never on the row count, so a row's value is bitwise the same alone, in any batch
// and at any position.
// ---------------------------------------------------------------------------------------
constexpr int kSweepMaxParams = 8;
constexpr uint64_t kSweepMaxRows = 1ull << 20;
constexpr int kSweepMaxGrid = 2048;  // gx, and about gx * gy
// Least samples per lane worth one more workgroup along x. Measured over {16, 64, 256, 1024}
// (profiles/r8/expr_sweep.md): below 256 the per-row reduction shows (many small rows are
// 3 % slower at 64, 14 % at 16), at 1024 a few middling rows leave most of the device idle.
constexpr uint64_t kSweepMinSamplesPerLane = 256;
// Partials held at once (doubles): rows beyond this many partials go in further chunks of
// max(kSweepMaxPartials / gx, 1) rows.
constexpr uint64_t kSweepMaxPartials = 1ull << 24;

// Kernel source for f(x, p0..p{nparams-1}); a pJ at or above nparams fails in the compiler.
std::string expr_sweep_source(const std::string& expr, int nparams);
// hipRTC compile for gfx950 (no device needed), cached per (expression, nparams).
std::string expr_sweep_compile(const std::string& expr, int nparams);

struct SweepShape {
  int gx = 1, gy = 1;
};
// Launch shape of a sweep of `rows` rows over n_local samples each (no device needed):
// gx = grid if given, else clamp(ceil(n_local / (256 * kSweepMinSamplesPerLane)), 1, 2048);
// gy = clamp(2048 / gx, 1, rows). Throws when a lane's share of n_local would not fit the
// kernel's 32-bit per-lane count.
SweepShape expr_sweep_shape(uint64_t n_local, uint64_t rows, int grid = 0);

// Parameter rows from a text file: one row per line, numbers separated by commas, semicolons
// or whitespace, # starts a comment (the --profile reader's rules). Every row has the same
// width (<= 8), returned in *nparams; row-major values. Errors name the file, line and row.
std::vector<double> load_param_rows(const std::string& path, int* nparams);
// "p0=LO:HI:COUNT": COUNT evenly spaced one-parameter rows from LO to HI inclusive.
std::vector<double> linspace_param_rows(const std::string& spec);

class ExprSweep {
 public:
  ExprSweep(const std::string& expr, int nparams, int device = 0, int grid = 0);
  ExprSweep(const ExprSweep&) = delete;
  ExprSweep& operator=(const ExprSweep&) = delete;
  // out[k] = h * scale * sum f(a + (i + off) h, params[k*nparams ..]) over samples
  // [begin, begin + count) of the n-sample rule on [a, b], for `rows` rows (params is
  // rows x nparams, row-major; rows is explicit because nparams may be 0). One upload of
  // the rows, one partials and one close launch (more only when rows * gx partials would
  // pass 2^24 doubles: then rows go in chunks), one all-reduce of the rows' values when
  // the communicator has more than one rank, one copy back, one sync.
  std::vector<double> integrate(const std::vector<double>& params, uint64_t rows, double a,
                                double b, uint64_t n, Rule rule, uint64_t begin, uint64_t count,
                                double scale = 1.0, const Comm* comm = nullptr);
  // Device ms per sweep over `iters` back-to-back sweeps (events; the rows are uploaded
  // once, before the clock). Hooks as in ExprIntegrator::time.
  double time(const std::vector<double>& params, uint64_t rows, double a, double b, uint64_t n,
              Rule rule, uint64_t begin, uint64_t count, int iters,
              const std::function<void()>& at_start = {},
              const std::function<void()>& at_end = {});
  const std::string& expression() const { return expr_; }
  int nparams() const { return nparams_; }

 private:
  void check(const std::vector<double>& params, uint64_t rows, uint64_t n, uint64_t begin,
             uint64_t count) const;
  void upload(const std::vector<double>& params, uint64_t rows, int gx, hipStream_t s);
  void enqueue(double a, double h, double off, uint64_t begin, uint64_t count, uint64_t rows,
               SweepShape shape, double scale, hipStream_t s);
  std::string expr_;
  int nparams_, device_, grid_;
  Stream stream_;
  DeviceBuffer<double> params_, partials_, out_;
  PinnedBuffer<double> host_params_, host_out_;
  Event e0_, e1_;
  detail::RtcModule module_;  // the last member: destroyed first (miint/expr_rtc.hpp)
};

// ---------------------------------------------------------------------------------------
// Running integrals: F_i = scale * h * sum_{j <= i} f(x_j) at every sample (or every
// `every`-th one) of a run-time integrand, in one call.
//
// The reference's second half (4main.c) integrates a profile to a curve; TrainScan does
// that for the velocity table. Here the integrand is any expression over x: the distance
// curve of a user's v(t), a CDF, an error function. Reduce-then-scan on the computed
// samples, three stream-ordered kernels around the expression (expr_scan.cpp):
//
//   miint_expr_scan_tile_sums    tiles of 4096 samples (256 threads x 16 consecutive ones);
//                                a workgroup walks a contiguous run of R tiles: per tile the
//                                sum S (compute only) -> L[t], the sum of the run's tiles
//                                before t, and A[b], the run's sum. At most 2048 runs: one
//                                workgroup per tile (244 141 of them at 1e9 samples) ran at
//                                the dispatch rate, 2.2x the time of an ExprIntegrator pass
//   miint_expr_scan_tile_prefix  one workgroup, a contiguous stretch of (at most two) runs
//                                per thread -> exclusive B[b] and the slice sum T;
//                                P[t] = B[t / R] + L[t] is tile t's exclusive prefix
//   (world > 1)                  allgather of one T per rank, launch_exclusive_carry -> C
//   miint_expr_scan_write        re-evaluates a tile, scans it and stores
//                                ((C + P[t]) + local) * (h * scale); every == 1: 16-byte
//                                stores through an LDS transpose; every > 1: 8-byte stores of
//                                the selected samples, tiles without one are not evaluated
//
// No workgroup waits on another (no tickets, no look-back, no timeout path): nothing depends
// on co-residency. The launch shape depends on `count` (and `every`) only and every sum has
// a fixed order, so results are bitwise reproducible. Sample i sits at
// x = fma((double)i + off, h, a), the bits ExprIntegrator gives it. Samples, tiles and output
// positions are 64-bit.
// ---------------------------------------------------------------------------------------
constexpr uint64_t EXPR_SCAN_TILE = 4096;            // 256 threads x 16 samples
constexpr uint64_t kExprScanMaxRuns = 2048;          // workgroups of the sums and write passes
constexpr uint64_t kExprScanMaxTiles = 1ull << 22;   // tiles of one launch (L: 32 MB)

// Kernel source / code object of the scan kernels for `expr` (as expr_source / expr_compile).
std::string expr_scan_source(const std::string& expr);
std::string expr_scan_compile(const std::string& expr);
struct ScanShape {
  uint64_t tiles = 0, run = 1, runs = 0;
};
// How a slice of `count` samples is dealt out (no device needed): tiles = ceil(count / 4096),
// run = R = max(ceil(tiles / 2048), 1) tiles per workgroup, runs = ceil(tiles / R). Throws
// past kExprScanMaxTiles tiles.
ScanShape expr_scan_shape(uint64_t count);
// Values a launch over samples [begin, begin + count) writes: those F_i with
// (i + 1) % every == 0, i the global sample index: floor((begin + count) / every) -
// floor(begin / every). No device needed.
uint64_t expr_scan_outputs(uint64_t begin, uint64_t count, uint64_t every);
// Throws, naming the numbers, unless [begin, begin + count) lies in [0, n) without wrapping,
// every >= 1, out_capacity holds the launch's outputs and the slice has at most
// kExprScanMaxTiles tiles. No device needed; nothing is launched after a refusal.
void expr_scan_check(uint64_t n, uint64_t begin, uint64_t count, uint64_t every,
                     uint64_t out_capacity);

struct ExprScanResult {
  double total = 0.0;      // scale * h * sum over the launch, or over all ranks' slices
  uint64_t outputs = 0;    // values written to out_device
  double device_ms = 0.0;  // events around the launch's kernels (and collectives)
};

class ExprScan {
 public:
  ExprScan(const std::string& expr, int device = 0);
  ExprScan(const ExprScan&) = delete;
  ExprScan& operator=(const ExprScan&) = delete;
  // Writes F_i = scale * h * sum_{begin <= j <= i} f(x_j) for the selected samples of
  // [begin, begin + count) to out_device (device memory, out_capacity doubles), in order.
  // With a communicator of more than one rank the ranks hold consecutive slices in rank
  // order, rank r's values carry the lower ranks' slice sums (added in rank order) and
  // `total` is the sum over all slices, the same double on every rank. Synchronous.
  ExprScanResult run(double a, double b, uint64_t n, Rule rule, uint64_t begin, uint64_t count,
                     uint64_t every, double* out_device, uint64_t out_capacity,
                     double scale = 1.0, const Comm* comm = nullptr);
  // Device ms per scan over `iters` back-to-back scans (events, no host sync between them).
  double time(double a, double b, uint64_t n, Rule rule, uint64_t begin, uint64_t count,
              uint64_t every, double* out_device, uint64_t out_capacity, int iters);
  const std::string& expression() const { return expr_; }

 private:
  void reserve(uint64_t tiles, int world);
  void enqueue_local(double a, double h, double off, uint64_t begin, uint64_t count,
                     hipStream_t s);
  void enqueue_write(double a, double h, double off, uint64_t begin, uint64_t count,
                     uint64_t every, const double* carry, double hs, double* out,
                     hipStream_t s);
  std::string expr_;
  int device_;
  Stream stream_;
  DeviceBuffer<double> local_;    // L[t]: grows on demand, kept across calls
  DeviceBuffer<double> runs_;     // A[b], then B[b]: 2 x kExprScanMaxRuns
  DeviceBuffer<double> scalars_;  // [0] T, [1] C, [2..) the ranks' gathered T
  PinnedBuffer<double> host_;           // the ranks' T (one without a communicator)
  Event e0_, e1_;
  detail::RtcModule module_;  // the last member: destroyed first (miint/expr_rtc.hpp)
};

// ---------------------------------------------------------------------------------------
// Double integrals: sum of f(x, y) over the nx x ny samples of a rectangle [ax, bx] x [ay, by]
// (the same rule on both axes), for one C++ expression over x and y.
//
// Through ExprSweep a double integral is f(x, p0) with one parameter row per y sample: at
// most 2^20 rows, the y values uploaded as data, every x coordinate formed again for every
// row, gx partials written and closed per row. Here a lane keeps a few columns in registers
// and runs down a contiguous stretch of rows (expr2d.cpp):
//
//   miint_expr2d_partials  256 lanes = lx along x by 256 / lx along y. An item is a column
//                          panel (lx * cpl columns, cpl <= 4 per lane) by a row stretch. A
//                          lane forms its columns' x once per item, then per row y once and
//                          per sample f and one add (cpl accumulators); what f does with x
//                          alone is hoisted out of the row loop by the compiler. A workgroup
//                          takes a contiguous run of items; block reduction -> one partial
//                          per workgroup
//   miint_expr2d_finalize  the closing step -> ((hx * hy) * scale) * sum
//
// Sample (i, j) sits at x_i = fma((double)i + off, hx, ax), y_j = fma((double)j + off, hy, ay):
// the bits ExprIntegrator gives a coordinate. A launch covers all nx columns of rows
// [row_begin, row_begin + row_count); ranks split the rows (rank_slice(ny, r, world)). The
// launch shape depends on (nx, row_count, grid) only and every sum has a fixed order:
// bitwise reproducible. No workgroup waits on another. Rows and flattened samples are 64-bit.
// ---------------------------------------------------------------------------------------
constexpr uint64_t kExpr2DMaxNx = (1ull << 32) - 1;
constexpr uint64_t kExpr2DMaxNy = 1ull << 40;
constexpr int kExpr2DMaxGrid = 2048;

std::string expr2d_source(const std::string& expr);
// hipRTC compile for gfx950 (no device needed), cached per expression.
std::string expr2d_compile(const std::string& expr);

struct Expr2DShape {
  int lanes_x = 1;             // lanes along x (a power of two; 256 / lanes_x along y)
  int cols_per_lane = 1;       // 1..4: a panel is lanes_x * cols_per_lane columns
  uint64_t rows_per_item = 1;  // rows of the longest stretch (the rows are dealt evenly)
  uint64_t stretches = 1, panels = 1;
  uint64_t items = 1;          // panels * stretches, item = panel * stretches + stretch
  uint64_t items_per_wg = 1;   // workgroup w takes items [w * items_per_wg, ...)
  int workgroups = 1;
  uint64_t lane_samples = 1;   // the largest per-lane sample count (32-bit in the kernel)
};
// How a launch over all nx columns of row_count rows is dealt out (no device needed; grid:
// the workgroup cap, 0 = 2048). A function of (nx, row_count, grid) only. For nx * row_count
// >= 2^20 more than half of workgroups * 256 * lane_samples are real samples. Throws, naming
// the numbers, when no shape keeps the per-lane count below 2^32.
Expr2DShape expr2d_shape(uint64_t nx, uint64_t row_count, int grid = 0);
// Throws, naming the numbers, unless 1 <= nx < 2^32, 1 <= ny <= 2^40, rows [row_begin,
// row_begin + row_count) lie in [0, ny) without wrapping and the shape exists. No device
// needed; nothing is launched after a refusal.
void expr2d_check(uint64_t nx, uint64_t ny, uint64_t row_begin, uint64_t row_count,
                  int grid = 0);
// expr2d_check, then the shape the launch of that slice uses: expr2d_shape(nx, row_count,
// grid), which row_begin never reaches (no items and no workgroups when row_count == 0).
// ExprIntegrator2D asks once per integrate / time call.
Expr2DShape expr2d_plan(uint64_t nx, uint64_t ny, uint64_t row_begin, uint64_t row_count,
                        int grid = 0);
namespace detail {
// expr_check with the expression itself named in the error (expr2d_source, HostExpr2D).
void expr_check_named(const std::string& expr);
}  // namespace detail

class ExprIntegrator2D {
 public:
  ExprIntegrator2D(const std::string& expr, int device = 0, int grid = 0);
  ExprIntegrator2D(const ExprIntegrator2D&) = delete;
  ExprIntegrator2D& operator=(const ExprIntegrator2D&) = delete;
  // S * ((hx * hy) * scale), S the sum of f(x_i, y_j) over all nx columns of rows
  // [row_begin, row_begin + row_count); row_count == 0 gives 0.0. With a communicator of
  // more than one rank the ranks' values are all-reduced. Synchronous.
  double integrate(double ax, double bx, uint64_t nx, double ay, double by, uint64_t ny,
                   Rule rule, uint64_t row_begin, uint64_t row_count, double scale = 1.0,
                   const Comm* comm = nullptr);
  // Device ms per integration over `iters` back-to-back ones; hooks as ExprIntegrator::time.
  double time(double ax, double bx, uint64_t nx, double ay, double by, uint64_t ny, Rule rule,
              uint64_t row_begin, uint64_t row_count, int iters,
              const std::function<void()>& at_start = {},
              const std::function<void()>& at_end = {});
  const std::string& expression() const { return expr_; }

 private:
  void enqueue(const Expr2DShape& sh, double ax, double hx, double ay, double hy, double off,
               uint64_t nx, uint64_t row_begin, uint64_t row_count, double scale,
               hipStream_t s);
  std::string expr_;
  int device_, grid_;
  Stream stream_;
  DeviceBuffer<double> partials_, out_;
  PinnedBuffer<double> host_;
  Event e0_, e1_;
  detail::RtcModule module_;  // the last member: destroyed first (miint/expr_rtc.hpp)
};

// ---------------------------------------------------------------------------------------
// Adaptive integration: the integral of f(x) on [a, b] to a requested tolerance, with an error
// estimate and a `converged` flag, the samples placed where the integrand needs them.
//
// Every family above sums n equally spaced samples and leaves n to the caller. Here the
// Gauss-Kronrod (7, 15) pair is applied to a list of intervals, and the intervals whose
// estimate misses their share of the tolerance are bisected, round by round (expr_adaptive.cpp,
// expr_adaptive_rounds.cpp).
// On [lo, hi] with hw = 0.5 (hi - lo), c = lo + hw and nodes x_j = fma(hw, t_j, c):
//   K = hw sum wk_j f(x_j) (15 nodes), G = hw sum wg_j f(x_j) (the 7 Gauss nodes among them),
//   R = hw sum wk_j |f(x_j)|, err = |K - G|. Neither endpoint is evaluated.
// The list starts as `panels` equal intervals (edges a + ((b - a) k) / panels, the last one b)
// and stays in x order. A round, over the whole active list of n intervals:
//
//   miint_adapt_eval     one interval per lane: K, err, R; one partial of K per workgroup
//   miint_adapt_close    one workgroup: sum_K in index order, t = rtol |S_acc + sum_K|,
//                        tol = atol > t ? atol : t (a NaN sum gives a NaN tolerance)
//   miint_adapt_decide   per interval, in this order: K or err not finite -> accept, counted
//                        in `nonfinite`; not (err > (tol w) / W), w = hi - lo, W = |b - a| ->
//                        accept (so a NaN tolerance accepts everything: the value is lost
//                        already); err <= 50 * 2^-52 R -> accept, counted in `floor` (rounding
//                        noise: bisection cannot improve it); depth >= max_depth, or c equal
//                        to lo or hi -> accept, counted in `forced`; else split. Per
//                        workgroup: the split count, the counters, the sums of the accepted
//                        K, err, R and of the K and err to be split
//   miint_adapt_prefix   one workgroup: exclusive prefix of the split counts, the round's sums
//                        in workgroup order onto S_acc, E_acc, R_acc, the round's record
//                        into pinned host memory. When the partition (the intervals accepted
//                        so far plus the next list) would pass max_intervals the round is
//                        `capped`: nothing is split, the pending K and err join the totals
//   miint_adapt_scatter  the children (lo, c), (c, hi) at depth + 1 take their parent's place in
//                        the other list (2 * exclusive prefix); the accepted intervals go to
//                        the caller's buffer if one was given
//
// The host side of the rounds is detail::AdaptRounds (miint/expr_rtc.hpp), which ExprAdaptiveOsc,
// ExprAdaptive2D and ExprAdaptiveRegion run around their own evaluation kernels too; the four
// kernels behind the evaluation are one text for intervals and rectangles (adapt_round_source).
// The host reads the record (the next count and the flags) after one sync per round and stops
// when the next list is empty or the round was capped. No workgroup waits on another, the launch
// shapes depend on the active count only and every sum has a fixed order: bitwise reproducible.
// a > b integrates [b, a] and negates the value; a == b gives 0 with no launch. The partition
// never passes max_intervals, so a caller's interval buffer of that capacity cannot overflow.
// ---------------------------------------------------------------------------------------
constexpr uint64_t kAdaptMaxIntervalsLimit = 1ull << 26;  // the lists alone are 2 GB there
constexpr int kAdaptMaxDepthLimit = 200;

// The one table of the rule. gk15_nodes(): the 15 Kronrod nodes on [-1, 1], ascending;
// gk15_weights(): their weights; gk7_weights(): the weights of the 7 Gauss nodes, which are
// nodes 1, 3, ..., 13. The generated source prints the same doubles as hex floats.
std::vector<double> gk15_nodes();
std::vector<double> gk15_weights();
std::vector<double> gk7_weights();
// The 15 nodes fma(hw, t_j, c) of [lo, hi], ascending: the bits the kernels evaluate f at.
void gk15_abscissae(double lo, double hi, double* x15);

// The panels a call starts from unless told. A round costs about 28 us whatever it holds (five
// launches and a sync) and 983040 evaluations cost what 3840 do, so starting fine saves rounds:
// against 256 and 4096, 65536 took 0.034 instead of 0.25 and 0.15 ms for 1.0/(x*x+1e-8) and
// the same time for exp(-x*x) and 1.0/sqrt(x) (profiles/r21/expr_adaptive.md).
constexpr uint64_t kAdaptDefaultPanels = 65536;

// ---------------------------------------------------------------------------------------
// Infinite and half-infinite ranges (opt-in: AdaptOptions::unbounded, AdaptSweepOptions::
// unbounded). QUADPACK's qagi map onto t in (0, 1]: infinity lands at t = 0, where doubles are
// densest and where the (7, 15) pair never puts a node. With
//   q = (1.0 - t) / t
// the rounds integrate g over t in [0, 1] instead of f over x:
//   (a, +inf), a finite   "upper"   x = a + q    g(t) = f(x) / (t * t)
//   (-inf, b), b finite   "lower"   x = b - q    g(t) = f(x) / (t * t)
//   (-inf, +inf)          "both"                 g(t) = (f(q) + f(-q)) / (t * t)
// q, x and g are formed in exactly this order, every operation rounded on its own (contraction
// off); f itself is compiled as for a finite range. The rounds are the finite rule's on [0, 1]
// with W = 1: the same panels, init edges, decision order, caps and counters; only the
// per-interval eval kernel has a twin per kind (miint_adapt_eval_upper / _lower / _both,
// miint_asweep_eval_upper / ...), generated into a second source that is compiled and loaded at
// an object's first unbounded call. So err_est, resabs and tol are those of g: resabs is the
// rule's integral of |g|, which for "both" is that of |f(x) + f(-x)| over (0, inf), not of |f|
// over the axis. The partition (intervals_out) is the partition of [0, 1] in t, ascending,
// whatever the order of a and b: it is what the kernels bisected; adapt_range_map gives the x.
// a = +inf with b finite, and the other swapped forms, negate the value as a > b does; a == b
// gives 0 with no launch, for infinite values too (range "finite"). NaN ends are refused, and
// so are finite ends whose b - a overflows. With `unbounded` false every check and message is
// that of the finite rule, and with it true finite ends run the finite path bit for bit: an
// infinity that reaches this layer from an overflowed computation is still caught, one that a
// caller typed (the CLIs and the integrate_* functions set the flag themselves) is not.
// Limits: an integrable singularity at the finite end sits at t = 1, where nodes soon round
// onto the end (exp(-x)/sqrt(x) on (0, inf) reports `nonfinite`: split it into a finite call on
// [0, 1] and (1, inf)); oscillatory tails such as sin(x)/x do not converge, and the run says so.
// ---------------------------------------------------------------------------------------
enum class AdaptRange { kFinite = 0, kUpper = 1, kLower = 2, kBoth = 3 };
// "finite", "upper", "lower", "both".
const char* adapt_range_name(AdaptRange kind);
// The kind of the range between a and b in either order (a == b and NaN ends: kFinite).
AdaptRange adapt_range(double a, double b);
// The map's three lines on the host, rounded as on the device, for n values of t: x[i] and the
// divisor jac[i] = t * t (g = f(x) / jac), and for kBoth x[i] = q, x2[i] = -q (g = (f(x) +
// f(x2)) / jac); x2 may be null otherwise. kFinite: x = t, jac = 1. The end used is the finite
// one of a, b. The numpy model evaluates f at these bits.
void adapt_range_map(double a, double b, const double* t, uint64_t n, double* x, double* jac,
                     double* x2);

struct AdaptOptions {
  double rtol = 1e-10, atol = 0.0;
  uint64_t panels = kAdaptDefaultPanels;
  int max_depth = 60;
  uint64_t max_intervals = 1ull << 22;
  bool unbounded = false;      // accept infinite ends (the map above)
};
struct AdaptResult {
  double value = 0.0, err_est = 0.0, resabs = 0.0;
  double tol = 0.0;            // the last round's tolerance
  bool converged = false;      // err_est <= tol, not capped, nonfinite == 0
  uint64_t evals = 0;          // 15 x intervals evaluated
  uint64_t rounds = 0, intervals = 0, splits = 0;
  uint64_t floor = 0, forced = 0, nonfinite = 0;
  bool capped = false;
  double device_ms = 0.0;      // events around the call's rounds
  std::string range = "finite";  // adapt_range_name of the call's range
};

// Throws, naming the numbers, unless a and b are finite (with opt.unbounded: not NaN, and
// b - a finite when both are), rtol and atol are >= 0 and not both 0, 1 <= max_intervals <=
// 2^26, 1 <= panels <= max_intervals and 0 <= max_depth <= 200. No device needed; nothing is
// launched after a refusal.
void adapt_check(double a, double b, const AdaptOptions& opt);
std::string expr_adapt_source(const std::string& expr);
// hipRTC compile for gfx950 (no device needed), cached per expression.
std::string expr_adapt_compile(const std::string& expr);
// The eval kernels of the three infinite kinds (the rest of a round is expr_adapt_source's).
std::string expr_adapt_unbounded_source(const std::string& expr);
std::string expr_adapt_unbounded_compile(const std::string& expr);
namespace detail {
// The rounds' job (miint/expr_rtc.hpp) for one dimension: [lo, hi], lo < hi, under opt.
AdaptJob adapt_job(double lo, double hi, const AdaptOptions& opt, double* out, uint64_t capacity,
                   bool descending = false);
}  // namespace detail

class ExprAdaptive {
 public:
  ExprAdaptive(const std::string& expr, int device = 0);
  ExprAdaptive(const ExprAdaptive&) = delete;
  ExprAdaptive& operator=(const ExprAdaptive&) = delete;
  // The integral of f on [a, b] by the rounds above. With intervals_out (device memory,
  // `capacity` pairs of doubles; refused up front unless capacity >= max_intervals) the final
  // partition is also stored there as (lo, hi) pairs running from a to b: result.intervals
  // of them. Synchronous: one sync per round.
  AdaptResult integrate(double a, double b, const AdaptOptions& opt = {},
                        double* intervals_out = nullptr, uint64_t capacity = 0);
  // Device ms per call over `iters` back-to-back calls (events around them; the rounds' syncs
  // and the host's reads between them are inside).
  double time(double a, double b, const AdaptOptions& opt, int iters);
  const std::string& expression() const { return expr_; }

 private:
  // A call's range as the rounds take it: the job, and the evaluation launch of its kind.
  detail::AdaptJob job(double a, double b, const AdaptOptions& opt, double* out,
                       uint64_t capacity);
  detail::AdaptRounds::Eval eval(double a, double b);
  std::string expr_;
  detail::AdaptRounds rounds_;  // with miint_adapt_eval
  // the last member, destroyed before the rounds' stream (miint/expr_rtc.hpp): the twins of the
  // infinite kinds, loaded at the first unbounded call
  std::unique_ptr<detail::RtcModule> unbounded_;
};

// ---------------------------------------------------------------------------------------
// Oscillatory weights: the integral of f(x) cos(omega x) or f(x) sin(omega x) on [a, b] to a
// requested tolerance, omega a number of the call and not part of f (QUADPACK's qawo), and the
// Fourier tail on (a, +inf) (its qawf). ExprAdaptive pays for an oscillatory factor in
// bisections: |K15 - G7| means nothing until an interval is shorter than a period. Here the
// rule is Filon-Clenshaw-Curtis: the weight is integrated exactly and only f is interpolated,
// so one interval may hold any number of periods (expr_adaptive_osc.cpp).
//
// On [lo, hi] with hw = 0.5 (hi - lo), c = lo + hw, the 25 Chebyshev extrema t_j = cos(j pi /
// 24), j = 0 (t = 1, the upper end) .. 24 (t = -1), the nodes x_j = fma(hw, t_j, c) and x_{24-j}
// = fma(hw, -t_j, c); the 13 even-numbered ones are the embedded coarse rule. Both ends are
// nodes. With l_j the Lagrange basis on the 25 (or the 13) nodes and par = omega hw:
//   Wc_j(par) = int_{-1}^{1} l_j(t) cos(par t) dt,   Ws_j(par) = int l_j(t) sin(par t) dt,
// Wc_{24-j} = Wc_j and Ws_{24-j} = -Ws_j (Ws_12 = 0), so the kernel works on mirrored pairs and
// half tables. Operation by operation, contraction off (miint_osc_rule):
//   f12 = f(c); for j = 11 down to 0: fp = f(fma(hw, t_j, c)), fm = f(fma(hw, -t_j, c)),
//     s = fp + fm, d = fp - fm, a = |fp| + |fm|
//   ic24 = Wc24_12 f12, then ic24 = fma(Wc24_j, s, ic24);  is24 = Ws24_11 d (at j = 11), then
//     is24 = fma(Ws24_j, d, is24);  ic12, is12 the same over the even j with Wc12, Ws12 (is12
//     starts at j = 10);  sa = w_12 |f12|, then sa = fma(w_j, a, sa), w the plain 25-point
//     Clenshaw-Curtis weights
//   p = omega c, e = fma(omega, c, -p) (the product's rounding error, exact), (S0, C0) =
//     sincos(p), S = fma(e, C0, S0), C = fma(-e, S0, C0): the phase omega c to about an ulp of S
//     and C, not to an ulp of p
//   cos: K = hw (C ic24 - S is24), G = hw (C ic12 - S is12)
//   sin: K = hw (S ic24 + C is24), G = hw (S ic12 + C is12)
//   err = |K - G|, R = hw sa: the rule's integral of |f| (it bounds that of |f w|) and feeds the
//   floor test unchanged.
// omega = 0 gives e = 0, S = 0, C = 1 exactly: plain Clenshaw-Curtis (25, 13) for cos, 0 for sin.
//
// The weights depend on par only, and the intervals of one depth share it. The nominal value
// is par_d = omega hw0 2^-d with hw0 = 0.5 ((b - a) / panels), halved exactly; the host builds
// one table per call, a row of kOscRow doubles per depth 0 .. max_depth (Wc24[13], Ws24[12],
// Wc12[7], Ws12[6], two of padding), uploads it, and the kernel indexes it by the interval's
// depth: no recurrence and no branch on par in the kernel, one path for every omega, 25
// evaluations, four dot products and one sincos a lane.
//
// osc_weights(par) on the host, in long double (64-bit significand), from the Chebyshev moments
// M_k = int T_k(t) exp(i par t) dt, k = 0 .. 24 (real for even k, imaginary for odd k):
//   |par| < 64: exp(i par t) = J_0 + 2 sum_n i^n J_n(par) T_n(t), J_n by Miller's backward
//     recurrence from n = 2 ceil(|par| / 2) + 96, normalised with J_0 + 2 sum J_2m = 1, and
//     int T_k T_n = 1 / (1 - (k + n)^2) + 1 / (1 - (k - n)^2) for k + n even, else 0. Every term
//     is bounded, and J_n has dropped far below 2^-64 where the series is cut.
//   |par| >= 64: by parts, M_k = (B_k - D_k) / (i par) with B_k = exp(i par) - (-1)^k exp(-i
//     par) and D_k = int T_k' exp(i par t) dt, D_1 = M_0 = 2 sin(par) / par, D_2 = 4 M_1,
//     D_{k+1} = (k + 1) (2 M_k + D_{k-1} / (k - 1)), forwards. An error in D_k is passed on times
//     2 (k + 1) / |par| < 1 for k <= 24: stable.
//   par = 0: M_k = 2 / (1 - k^2), k even.
// Then W_j = (2 / N) c_j sum''_k cos(j k pi / N) M_k (c_j = 1/2 at the ends, the first and last
// term of the sum halved), N = 24 and 12, rounded to double. Wc is even and Ws odd in par.
// tests/test_expr_osc_cpu.py holds them to 50-digit values.
//
// Limits. Both ends of every interval are evaluated, so f must be finite on the closed range:
// an end singularity (1.0/sqrt(x) from 0) reports `nonfinite`, and the "singular end" advice of
// the Gauss-Kronrod rule does not carry over. The intervals' widths differ from the nominal
// hw0 2^-d by the rounding of their ends, about 2^-53 max|x|, so par is off by |omega| times
// that, and the nodes' rounding moves the weight's phase by as much: the value is uncertain by
// about |omega| max|x| 2^-53 relative to the intervals' own contributions, whatever the
// tolerance asked. omega and the ends must be finite; a > b negates; a == b gives 0 with no
// launch.
//
// The Fourier tail (b = +inf, omega != 0), a host loop over the finite rule: cycles of length
// L = (2 floor(|omega|) + 1) pi / |omega| from a, cycle k = 1, 2, ... one finite call on [a +
// (k - 1) L, a + k L] from OscTailOptions::panels panels with rtol = 0 and atol (1 - p) p^(k -
// 1), p = 0.9. From 3 cycles on Wynn's epsilon algorithm runs on the partial sums; the
// extrapolation's estimate is |e_k - e_{k-1}| + |e_k - e_{k-2}| over its last three results (so
// from cycle 5). The loop stops when (the sum of the cycles' err_est) + 50 |cycle k| <= atol
// (the sum itself has converged: `extrapolated` false), when (that sum) + (the extrapolation's
// estimate) <= atol (`extrapolated` true, the value is e_k), or at max_cycles. err_est is the
// sum of the cycles' estimates plus the estimate of whichever stopped it. `converged` further
// asks that every cycle converged and that f decays: the last cycle's R must be below the first
// one's (f = 1.0 sums to 0 in Abel's sense; the run ends `no decay` instead). atol > 0 is
// required.
// ---------------------------------------------------------------------------------------
constexpr int kOscRow = 40;  // doubles per depth: Wc24[13], Ws24[12], Wc12[7], Ws12[6], 2 unused
enum class OscKind { kCos = 0, kSin = 1 };
// "cos" or "sin"; osc_kind throws on any other name.
const char* osc_kind_name(OscKind kind);
OscKind osc_kind(const std::string& name);
// t_j = cos(j pi / 24), j = 0 .. 24 (descending from 1 to -1), and the plain Clenshaw-Curtis
// weights of those nodes: the doubles the generated source prints.
std::vector<double> osc_nodes();
std::vector<double> osc_cc_weights();
// Wc24[25], Ws24[25], Wc12[13], Ws12[13] in that order (76 doubles), node order as osc_nodes()
// (the 13-node rule on its even ones). Throws unless par is finite.
std::vector<double> osc_weights(double par);
// The row of the device table for par: the half tables, kOscRow doubles.
void osc_table_row(double par, double* row);
// The 25 nodes of [lo, hi] in the order of osc_nodes(): the bits the kernels evaluate f at.
void osc_abscissae(double lo, double hi, double* x25);

struct OscTailOptions {
  uint64_t panels = 16;   // per cycle
  int max_cycles = 50;
};
struct OscResult : AdaptResult {
  double omega = 0.0;
  std::string kind = "cos";
  uint64_t cycles = 0;         // the Fourier tail's finite calls; 0 for a finite range
  bool extrapolated = false;   // the value is the epsilon algorithm's
  std::string reason;          // why a run did not converge ("" when it did)
};

// adapt_check on the ends (b = +inf is taken with `tail`), omega finite; for the tail also
// omega != 0, a finite, atol > 0, 1 <= max_cycles <= 10000 and the cycle's panels.
void osc_check(double a, double b, double omega, const AdaptOptions& opt, bool tail = false,
               const OscTailOptions& topt = {});
// The two evaluation twins, miint_osc_eval_cos and miint_osc_eval_sin (the other kernels of a
// round are expr_adapt_source's, unchanged).
std::string expr_osc_source(const std::string& expr);
std::string expr_osc_compile(const std::string& expr);
// Wynn's epsilon algorithm on the sequence s[0 .. n), n >= 3: the last entry of the highest
// even column. Plain doubles in a fixed order (the numpy model repeats it).
double osc_epsilon(const double* s, int n);
// Why a finished finite run did not converge ("" when it did), from its counters.
std::string osc_reason(const AdaptResult& r);

class ExprAdaptiveOsc {
 public:
  ExprAdaptiveOsc(const std::string& expr, int device = 0);
  // The integral of f(x) cos(omega x) (or sin) on [a, b] by the rounds of intervals
  // (detail::AdaptRounds, ExprAdaptive's) around the rule above; intervals_out as
  // ExprAdaptive::integrate. evals counts 25 per interval.
  OscResult integrate(double a, double b, double omega, OscKind kind, const AdaptOptions& opt = {},
                      double* intervals_out = nullptr, uint64_t capacity = 0);
  // The same on (a, +inf) by the cycles above. opt.panels is not used (topt.panels is).
  OscResult integrate_tail(double a, double omega, OscKind kind, const AdaptOptions& opt,
                           const OscTailOptions& topt = {});
  double time(double a, double b, double omega, OscKind kind, const AdaptOptions& opt, int iters);
  const std::string& expression() const { return expr_; }
  uint64_t table_uploads() const { return uploads_; }

 private:
  void upload(double par0, int rows, int upto);
  AdaptResult run(const detail::AdaptJob& job, double hw0, double omega, OscKind kind, bool timed);
  std::string expr_;
  detail::AdaptRounds rounds_;  // expr_adapt_source's module: its evaluation kernel is not used
  DeviceBuffer<double> table_;          // (max_depth + 1) x kOscRow
  std::vector<double> host_table_;
  double table_par0_ = 0.0;
  int table_rows_ = 0;                  // rows allocated
  int table_depths_ = 0;                // rows 0 .. table_depths_ - 1 hold table_par0_'s weights
  uint64_t uploads_ = 0;
  detail::RtcModule twins_;  // the last member: destroyed first (miint/expr_rtc.hpp)
};

// ---------------------------------------------------------------------------------------
// Adaptive double integrals: the integral of f(x, y) over a finite rectangle [ax, bx] x [ay, by]
// to max(atol, rtol |value|), with an error estimate and a `converged` flag.
//
// ExprIntegrator2D sums nx x ny equally spaced samples and leaves both to the caller. Here the
// tensor product of the (7, 15) pair above is applied to a list of rectangles, and a rectangle
// whose estimate misses its share (by area) of the tolerance is bisected along the axis that
// carries more of the error, round by round (expr_adaptive2d.cpp).
//
// Per rectangle [x0, x1] x [y0, y1], 225 evaluations, none on an edge:
//   hx = 0.5 (x1 - x0), cx = x0 + hx, x nodes cx and fma(hx, -+t_i, cx); the same in y.
//   Row at y node j (the 1-D order: the centre, then the pairs (-t_i, +t_i) outwards, by fma):
//     rk_j = sum_i wk_i f,  rg_j = sum_{i Gauss} wg_i f,  ra_j = sum_i wk_i |f|
//     centre: rk = wk_0 f0, rg = wg_0 f0, ra = wk_0 |f0|;
//     pair i: rk = fma(wk_i, f1 + f2, rk), ra = fma(wk_i, |f1| + |f2|, ra), and for the even
//     (Gauss) i rg = fma(wg_i, f1 + f2, rg), f1 at -t_i and f2 at +t_i.
//   The rows are combined in the same order over j: the centre row first, then per pair the
//   two rows' sums added (the row at -t_j first) and carried by fma:
//     KK = sum_j wk_j rk_j,  GK = sum_j wk_j rg_j,  RA = sum_j wk_j ra_j   (all j)
//     GG = sum_j wg_j rg_j,  KG = sum_j wg_j rk_j                          (the even, Gauss j)
//   With s = hx * hy: K = s KK, err = |s KK - s GG|, ex = |s KK - s GK| (the Gauss rule along x
//   only: the x direction's error), ey = |s KK - s KG|, R = s RA. Contraction is off where
//   these are rounded and compared, as in miint_gk15.
// Split axis: x if ex > ey, y if ey > ex; on a tie x when wx * Wy >= wy * Wx (the relatively
// wider side), else y; w the rectangle's sides, W the box's.
// Decision, in this order: K or err not finite -> accept, counted in `nonfinite`;
// not (err > (tol (wx wy)) / (Wx Wy)) -> accept; err <= 50 * 2^-52 R -> accept, `floor`; the
// chosen axis's own depth >= max_depth, or its midpoint equal to one of its ends -> accept,
// `forced`; else bisect along the chosen axis, the children taking slots 2 p and 2 p + 1 of the
// next list (p: the rectangles split before it). A rectangle carries one depth per axis (the
// halves of one 32-bit word).
//
// The list starts as panels_x x panels_y equal rectangles, x fastest, each axis's edges formed
// as miint_adapt_init forms them. A round is ExprAdaptive's, run by the same engine
// (detail::AdaptRounds in two dimensions) on the same text: miint_adapt2d_eval (one rectangle
// per lane; the loop over the 15 rows is rolled, a row's 15 evaluations unrolled in it),
// _close (sum_K and tol = max(atol, rtol |S_acc + sum_K|) on the device), _decide, _prefix
// (the cap: accepted + (n - splits) + 2 splits > max_intervals splits nothing and the pending
// sums join the totals; the eighteen-word record: ExprAdaptive's sixteen, then splits_x and
// splits_y) and _scatter; one sync per round, at most 2 max_depth + 1 rounds, no workgroup
// waits on another, every sum in an order fixed by the list length: bitwise reproducible.
// ax > bx negates, ay > by negates; either pair equal gives 0 with no launch. Infinite sides,
// parameter rows and more than one rank are left out.
// A limit: a discontinuity along a curve leaves err proportional to the area of the rectangles
// it cuts, so their share of the tolerance is never met: such a run ends `capped` (an
// indicator's tool is the fixed rule or the lattice). A point or edge singularity is resolved
// as far as the doubles go, at up to 61 (one axis) or 121 rounds.
// ---------------------------------------------------------------------------------------
constexpr uint64_t kAdapt2DDefaultPanels = 64;  // per axis: 4096 rectangles, 921 600 evaluations

struct Adapt2DOptions {
  double rtol = 1e-10, atol = 0.0;
  uint64_t panels_x = kAdapt2DDefaultPanels, panels_y = kAdapt2DDefaultPanels;
  int max_depth = 60;          // per axis
  uint64_t max_intervals = 1ull << 22;
};
struct Adapt2DResult {
  double value = 0.0, err_est = 0.0, resabs = 0.0;
  double tol = 0.0;            // the last round's tolerance
  bool converged = false;      // err_est <= tol, not capped, nonfinite == 0
  uint64_t evals = 0;          // 225 x rectangles evaluated
  uint64_t rounds = 0, intervals = 0, splits = 0;
  uint64_t splits_x = 0, splits_y = 0;  // splits = splits_x + splits_y
  uint64_t floor = 0, forced = 0, nonfinite = 0;
  bool capped = false;
  double device_ms = 0.0;      // events around the call's rounds
};

// Throws, naming the numbers, unless the four ends, both widths and the area are finite, rtol
// and atol are >= 0 and not both 0, 1 <= max_intervals <= 2^26, panels_x, panels_y >= 1 with
// panels_x * panels_y <= max_intervals, and 0 <= max_depth <= 200. No device needed; nothing
// is launched after a refusal.
void adapt2d_check(double ax, double bx, double ay, double by, const Adapt2DOptions& opt);
std::string expr_adapt2d_source(const std::string& expr);
// hipRTC compile for gfx950 (no device needed), cached per expression.
std::string expr_adapt2d_compile(const std::string& expr);

class ExprAdaptive2D {
 public:
  ExprAdaptive2D(const std::string& expr, int device = 0);
  ExprAdaptive2D(const ExprAdaptive2D&) = delete;
  ExprAdaptive2D& operator=(const ExprAdaptive2D&) = delete;
  // The integral of f over the rectangle by the rounds above. With rects_out (device memory,
  // `capacity` x 4 doubles; refused up front unless capacity >= max_intervals) the final
  // partition is also stored there as (x0, x1, y0, y1) with x0 < x1 and y0 < y1, ordered by
  // (y0, x0): result.intervals of them. Synchronous: one sync per round.
  Adapt2DResult integrate(double ax, double bx, double ay, double by,
                          const Adapt2DOptions& opt = {}, double* rects_out = nullptr,
                          uint64_t capacity = 0);
  // Device ms per call over `iters` back-to-back calls (events around them; the rounds' syncs
  // and the host's reads between them are inside).
  double time(double ax, double bx, double ay, double by, const Adapt2DOptions& opt, int iters);
  const std::string& expression() const { return expr_; }

 private:
  std::string expr_;
  detail::AdaptRounds rounds_;  // with miint_adapt2d_eval
};
namespace detail {
// ExprAdaptive2D::integrate and ::time on `rounds` (two dimensions), whose own evaluation kernel
// takes miint_adapt2d_eval's arguments: the checks, the ends' order and sign, the rounds.
Adapt2DResult adapt2d_integrate(AdaptRounds& rounds, double ax, double bx, double ay, double by,
                                const Adapt2DOptions& opt, double* rects_out, uint64_t capacity);
double adapt2d_time(AdaptRounds& rounds, double ax, double bx, double ay, double by,
                    const Adapt2DOptions& opt, int iters);
}  // namespace detail

// ---------------------------------------------------------------------------------------
// Adaptive double integrals between two curves: the integral of f(x, y) over the region
// { ax <= x <= bx, g(x) <= y <= h(x) } to max(atol, rtol |value|), g = ylo and h = yhi two more
// run-time expressions over x alone.
//
// The region is mapped onto (x, v) in [ax, bx] x [0, 1] by y = g(x) + (h(x) - g(x)) v, and
// the rounds of rectangles (detail::AdaptRounds, ExprAdaptive2D's) run on the mapped integrand
// f(x, y(x, v)) (h(x) - g(x)) over that rectangle. A rectangle of the list is [x0, x1] x
// [v0, v1]; the list starts as panels_x x panels_y equal rectangles of [min(ax, bx), max(ax, bx)]
// x [0, 1], formed by miint_adapt2d_init. Per rectangle (expr_adaptive_region.cpp,
// miint_region_gk15x15):
//   the x nodes x_i are ExprAdaptive2D's: cx and fma(hx, -+t_i, cx); the v nodes v_j are what it
//   forms along y: cy and fma(hy, -+t_j, cy).
//   Per x node, once per rectangle and in front of the loop over the rows:
//     g_i = ylo(x_i),  w_i = yhi(x_i) - g_i.
//   Per node pair: y_ij = fma(w_i, v_j, g_i), and the value summed is f(x_i, y_ij) * w_i.
//   Contraction is off around the subtraction and the product, as in miint_gk15x15.
// Everything after the 225 values is ExprAdaptive2D's with Wx = |bx - ax| and Wy = 1: the row
// sums, the row combination, K, err, ex, ey, R, the split axis, the decision order, the depths,
// the cap and the eighteen-word record. Of a round's six kernels only the evaluation kernel has
// a twin (miint_region_eval); the other five are the text ExprAdaptive2D compiles
// (adapt_round_source), around an engine of its own.
//
// ax > bx negates; ax == bx gives 0 with no launch. Where h(x) < g(x), w_i is negative and that
// strip counts negatively: the pointwise form of ay > by, neither refused nor clamped. A limit
// that is not finite at a node makes that rectangle `nonfinite`, as a non-finite f does.
// err_est, resabs and tol are those of the mapped integrand: resabs is the rule's integral of
// |f (h - g)|. With rects_out the partition is in (x, v), ordered by (v0, x0).
// Left out: limits in x that depend on y (swap the names), infinite sides, parameter rows, more
// than one rank, a host engine. A limit: a singularity of f on the boundary curve itself
// evaluates 0 * inf at nodes where w_i rounds to 0 and the run reports `nonfinite`
// (1.0/sqrt(y) over the upper half disc); one strictly inside the region that the map does not
// remove (1.0/sqrt(x*x+y*y) over the whole disc) runs to the cap: split the region there.
// ---------------------------------------------------------------------------------------
// Throws unless all three pass expr_check (naming which of the three it is and the expression)
// and neither limit mentions the identifier y.
std::string expr_region_source(const std::string& expr, const std::string& ylo,
                               const std::string& yhi);
// hipRTC compile for gfx950 (no device needed), cached per source.
std::string expr_region_compile(const std::string& expr, const std::string& ylo,
                                const std::string& yhi);

class ExprAdaptiveRegion {
 public:
  ExprAdaptiveRegion(const std::string& expr, const std::string& ylo, const std::string& yhi,
                     int device = 0);
  // As ExprAdaptive2D::integrate on [ax, bx] x [0, 1] in (x, v); the options are checked by
  // adapt2d_check with ay = 0, by = 1. rects_out takes (x0, x1, v0, v1), ordered by (v0, x0).
  Adapt2DResult integrate(double ax, double bx, const Adapt2DOptions& opt = {},
                          double* rects_out = nullptr, uint64_t capacity = 0);
  double time(double ax, double bx, const Adapt2DOptions& opt, int iters);
  const std::string& expression() const { return expr_; }
  const std::string& y_lo() const { return ylo_; }
  const std::string& y_hi() const { return yhi_; }

 private:
  std::string expr_, ylo_, yhi_;
  detail::AdaptRounds rounds_;  // with miint_region_eval
};

// ---------------------------------------------------------------------------------------
// Adaptive sweeps: f(x, p0..p{nparams-1}) on a shared [a, b] for K parameter rows, each row to
// its own tolerance max(atol, rtol |value of that row|), in shared rounds.
//
// Row r is treated exactly as ExprAdaptive treats its one integral: `panels` equal intervals
// with the same edges, the same (7, 15) pair on the same node bits in the same order (the two
// sources share miint_gk15's text), the same decisions in the same order against the row's own
// tol = max(atol, rtol |S_acc(r) + sum_K(r)|) and the shared width W = |b - a|, the same
// bisection, and the same cap: when the row's accepted intervals plus its next list would pass
// max_intervals (per row) the row's round is capped, nothing of the row is split and its
// pending K and err join its totals. Other rows do not notice.
//
// All rows' active intervals form one list sorted by (row, x), so a row is a contiguous segment
// (start, length), and the active rows form a compacted list in row order. A round, over the n
// active intervals of the na active rows (expr_adaptive_sweep.cpp):
//
//   miint_asweep_eval     one interval per lane: the row's parameters by the interval's row
//                         index, then K, err, R
//   miint_asweep_row      one wave per active row, no LDS, no barrier. sum_K: lane l chains
//                         elements l, l + 64, ... of the segment in index order from 0.0, then
//                         the 64-lane butterfly (xor 32, 16, ..., 1). The tolerance, then the
//                         decision per interval in chunks of 64 in index order: a split interval
//                         gets its rank among the row's splits (ballot and popcount, exact); the
//                         five sums (accepted K, err, R, pending K, err) each in the order of
//                         sum_K. Lane 0 closes the row's round: capped or not, the totals
//                         (S_acc += accepted K, + pending K when capped, as ExprAdaptive adds
//                         them), the counters, the row's next length
//   miint_asweep_prefix   one workgroup: exclusive prefix over the active rows of their next
//                         lengths (integers) -> every row's next segment start, the next list of
//                         active rows in row order, and the record (the next total and active
//                         count) into pinned host memory
//   miint_asweep_scatter  one interval per lane: children (lo, c), (c, hi) at depth + 1 to slots
//                         start(row) + 2 rank, + 1 of the other list, unless the row was capped
//
// Every floating-point sum of a row is formed from the row's own segment by the row's own wave,
// in an order that is a function of the segment's length only: a row's value, err_est, resabs,
// tol, counters and round count are bitwise the same alone, in any batch and at any position.
// A NaN stays in its row's state. What crosses rows is integer bookkeeping. Kernels are
// separated by launches; no workgroup waits on another and there is no floating-point atomic.
// The host reads the record after one sync per round and stops when no row is active; the
// per-row results are read back once after the last round.
//
// rows * max_intervals <= max_total (the capacity of the two lists) is checked up front and a
// row's next list never passes its cap, so the lists cannot overflow. a > b integrates [b, a]
// and negates every value; a == b gives K zero rows with no launch; rows == 0 an empty result.
// With AdaptSweepOptions::unbounded the shared range may be infinite: the rows run on t in
// [0, 1] over the mapped integrand (AdaptRange above), the eval kernel replaced by its twin.
// Left out: the final partition, multi-rank runs.
//
// Per-row ranges (integrate_ranges): row r integrates over its own [a_r, b_r] to its own
// max(atol, rtol |value of row r|), and is in every field, bit for bit, row 0 of
// integrate({p_r}, 1, a_r, b_r, opt) with the same resolved panels and max_intervals. The
// evaluation, prefix and scatter kernels are the first module's own; what reads the range has a
// twin, generated into a second source (expr_adapt_sweep_ranges_source, which holds no
// integrand: one text for every expression) that is compiled and loaded at an object's first
// ranged call:
//
//   miint_asweep_init_ranges  miint_asweep_init with a and b of row r read from the device
//                             arrays lo[r], hi[r] (lo[r] < hi[r]): w = hi[r] - lo[r], edges
//                             lo[r] + (w j) / panels, the last one hi[r]; the same segments and
//                             list of active rows
//   miint_asweep_row_ranges   miint_asweep_row with W and atol of the wave's row read from the
//                             device arrays width[r] (the host's hi_r - lo_r, as the shared
//                             range's W is the host's hi - lo) and atol[r]; otherwise the same
//                             text in the same order, so equal inputs give equal bits
//
// a_r > b_r integrates [b_r, a_r] and negates that row only. A row with a_r == b_r is 0 with
// tol = atol, converged, no evaluations: the host leaves it out of the launch (the device sees
// the other rows, compacted in order) and fills it in. NaN or infinite ends and a b_r - a_r
// that overflows are refused up front, naming the row, and so is `unbounded`.
// Left out: per-row infinite ranges.
// ---------------------------------------------------------------------------------------
constexpr uint64_t kAdaptSweepMaxTotalLimit = 1ull << 26;
constexpr uint64_t kAdaptSweepInitialTotal = 65536;  // rows * panels the default aims at
constexpr uint64_t kAdaptSweepMinPanels = 16;

struct AdaptSweepOptions {
  double rtol = 1e-10, atol = 0.0;
  uint64_t panels = 0;         // 0: adapt_sweep_default_panels(rows)
  int max_depth = 60;
  uint64_t max_intervals = 0;  // per row; 0: max_total / rows
  uint64_t max_total = 1ull << 22;
  bool unbounded = false;      // accept infinite ends of the shared range (see AdaptOptions)
};
struct AdaptSweepResult {
  std::string range = "finite";  // adapt_range_name of the call's shared range
  // per row
  std::vector<double> value, err_est, resabs, tol;
  std::vector<uint8_t> converged, capped;
  std::vector<uint64_t> evals, rounds, intervals, splits, floor, forced, nonfinite;
  // for the call
  uint64_t call_rounds = 0;  // the maximum over rows
  uint64_t call_evals = 0;   // the sum over rows
  uint64_t peak = 0;         // the longest whole list
  double device_ms = 0.0;
  uint64_t rows() const { return value.size(); }
};

// panels = 0: the largest power of two p <= 65536 with rows * p <= 65536, at least 16.
uint64_t adapt_sweep_default_panels(uint64_t rows);
// The options with the two zeros resolved, after every refusal (no device needed; throws
// naming the numbers): rows <= 2^20, nparams 0..8, param_count == rows * nparams,
// 1 <= max_total <= 2^26, then adapt_check on the resolved panels and max_intervals (so
// panels > max_intervals is refused there), then rows * max_intervals <= max_total.
AdaptSweepOptions adapt_sweep_check(uint64_t rows, int nparams, uint64_t param_count, double a,
                                    double b, const AdaptSweepOptions& opt);
// Kernel source for f(x, p0..p{nparams-1}); a pJ at or above nparams fails in the compiler.
std::string expr_adapt_sweep_source(const std::string& expr, int nparams);
// hipRTC compile for gfx950 (no device needed), cached per (expression, nparams).
std::string expr_adapt_sweep_compile(const std::string& expr, int nparams);
// The eval kernels of the three infinite kinds (the rest of a round is expr_adapt_sweep_source's).
std::string expr_adapt_sweep_unbounded_source(const std::string& expr, int nparams);
std::string expr_adapt_sweep_unbounded_compile(const std::string& expr, int nparams);
// adapt_sweep_check for per-row ranges: the same checks in the same words where they apply
// (rows, nparams, param_count, max_total, panels, rows * max_intervals, the tolerances, the
// depth), and a.size() == b.size() == rows, `unbounded` refused, every row's ends finite with a
// finite b_r - a_r (the first offending row is named). No device needed.
AdaptSweepOptions adapt_sweep_ranges_check(uint64_t rows, int nparams, uint64_t param_count,
                                           const std::vector<double>& a,
                                           const std::vector<double>& b,
                                           const AdaptSweepOptions& opt);
// The twins that read per-row ranges, and miint_acurve_prefix (ExprAdaptiveCurve below). No
// integrand is in it: one source and one compile (cached) for every expression.
std::string expr_adapt_sweep_ranges_source();
std::string expr_adapt_sweep_ranges_compile();

class ExprAdaptiveCurve;
struct AdaptCurveResult;

class ExprAdaptiveSweep {
 public:
  ExprAdaptiveSweep(const std::string& expr, int nparams, int device = 0);
  ExprAdaptiveSweep(const ExprAdaptiveSweep&) = delete;
  ExprAdaptiveSweep& operator=(const ExprAdaptiveSweep&) = delete;
  // The integrals of f(x, params[k * nparams ..]) on [a, b] for `rows` rows (params is rows x
  // nparams, row-major; rows is explicit because nparams may be 0). Synchronous: one sync per
  // round, one copy back of the rows' results at the end.
  AdaptSweepResult integrate(const std::vector<double>& params, uint64_t rows, double a, double b,
                             const AdaptSweepOptions& opt = {});
  // Device ms per call over `iters` back-to-back calls (events around them; the rows are
  // uploaded once, before the clock; the rounds' syncs and the host's reads are inside).
  double time(const std::vector<double>& params, uint64_t rows, double a, double b,
              const AdaptSweepOptions& opt, int iters);
  // Row r on its own [a[r], b[r]] (the block above): a and b hold `rows` doubles each.
  AdaptSweepResult integrate_ranges(const std::vector<double>& params, uint64_t rows,
                                    const std::vector<double>& a, const std::vector<double>& b,
                                    const AdaptSweepOptions& opt = {});
  // `time` for per-row ranges: the rows and their ranges are uploaded once, before the clock.
  double time_ranges(const std::vector<double>& params, uint64_t rows,
                     const std::vector<double>& a, const std::vector<double>& b,
                     const AdaptSweepOptions& opt, int iters);
  const std::string& expression() const { return expr_; }
  int nparams() const { return nparams_; }

 private:
  friend class ExprAdaptiveCurve;
  struct Call {
    uint64_t rounds = 0, evals = 0, peak = 0;
  };
  void reserve(uint64_t max_total, uint64_t rows);
  void upload(const std::vector<double>& params);
  Call rounds(double lo, double hi, uint64_t rows, const AdaptSweepOptions& opt,
              AdaptRange kind = AdaptRange::kFinite, double end = 0.0, bool ranged = false);
  void load_unbounded();
  void load_ranges();
  void reserve_curve(uint64_t points);
  // The rows with a_r != b_r in order, their parameters, lo < hi and per-row atol uploaded;
  // returns their indices. `atol` is null (opt.atol for every row) or one value per row.
  std::vector<uint64_t> upload_ranges(const std::vector<double>& params, uint64_t rows,
                                      const std::vector<double>& a, const std::vector<double>& b,
                                      const double* atol, const AdaptSweepOptions& opt);
  // integrate_ranges on options already resolved and checked; with `curve`, miint_acurve_prefix
  // runs behind the last round, inside the events (every row is live then).
  AdaptSweepResult run_ranges(const std::vector<double>& params, uint64_t rows,
                              const std::vector<double>& a, const std::vector<double>& b,
                              const double* atol, const AdaptSweepOptions& opt,
                              AdaptCurveResult* curve);
  void read_row(const unsigned long long* words, bool swapped, uint64_t k,
                AdaptSweepResult* r) const;
  std::string expr_;
  int nparams_, device_;
  Stream stream_;
  uint64_t reserved_ = 0, reserved_rows_ = 0;
  DeviceBuffer<double> params_;
  DeviceBuffer<double> list_[2];         // (lo, hi) pairs: 2 x max_total doubles each
  DeviceBuffer<unsigned> depth_[2], row_[2];  // per interval: its depth and its row
  DeviceBuffer<double> k_, err_, r_;     // per interval
  DeviceBuffer<unsigned> rank_;          // per interval: its rank among the row's splits, or none
  DeviceBuffer<unsigned> active_[2];     // the active rows in row order
  DeviceBuffer<unsigned> seg_start_, seg_len_, next_len_;  // per row / per active slot
  DeviceBuffer<unsigned long long> state_;   // 16 words per row (expr_adaptive_sweep.cpp)
  PinnedBuffer<unsigned long long> record_;  // the next total and active count
  uint64_t reserved_ranges_ = 0, reserved_curve_ = 0;
  DeviceBuffer<double> ranges_;       // per-row ranges: lo, hi, width, atol, 4 x rows doubles
  DeviceBuffer<double> curve_;        // F, err_est, tol, resabs: 4 x (M + 1) doubles
  DeviceBuffer<unsigned> curve_bad_;  // the unconverged cells before each point: M + 1
  PinnedBuffer<unsigned long long> curve_totals_;  // four doubles and the count
  Event e0_, e1_;
  detail::RtcModule module_;  // the last members: destroyed first (miint/expr_rtc.hpp)
  std::unique_ptr<detail::RtcModule> unbounded_;  // loaded at the first unbounded call
  std::unique_ptr<detail::RtcModule> ranged_;     // loaded at the first ranged call
};

// ---------------------------------------------------------------------------------------
// The running integral to a tolerance: F_j = the integral of f from x_0 to x_j on a caller's
// grid x_0, ..., x_M (strictly increasing or strictly decreasing, 1 <= M <= 2^20), F_0 = 0.
//
// Cell c = [x_c, x_{c+1}] is row c of a ranged sweep with nparams = 0, to its own tolerance
// max(atol_c, rtol |I_c|) with
//   atol_c = (atol * |x_{c+1} - x_c|) / |x_M - x_0|
// formed on the host in exactly that order: each cell is bitwise the single-row call on its
// range with atol = atol_c. So |F_j - true| is estimated by err_est_j, the sum of the cells'
// err_est before j, and that estimate is held to tol_j, the sum of their tol, which is at most
// atol + rtol * (the integral of |f| up to x_j): for a positive density every point of the CDF,
// the far tail included, is relatively accurate. converged_j: every cell before j converged. A
// capped or non-finite cell marks the points from it onwards and no point before it.
//
//   miint_acurve_prefix  one workgroup of 256 threads behind the last round. per =
//                        ceil(M / 256); thread t owns cells [t per, min((t + 1) per, M)) and
//                        chains their value (negated first on a descending grid), err_est, tol
//                        and resabs from 0.0 in index order, and counts its unconverged cells
//                        (err_est <= tol, not capped, nonfinite == 0, as the host decides it);
//                        thread 0 forms the 256 runs' exclusive prefixes P_t sequentially from
//                        0.0; every thread walks its run again: F_{j+1} = P_t + (its chain
//                        through cell j). M + 1 entries per array on the device, entry 0 zero;
//                        the totals go to pinned host memory
//
// No floating-point atomic, no waiting between workgroups, a fixed order: bitwise
// reproducible, and with M <= 256 (per = 1) the plain chain ((0 + I_0) + I_1) + ...
//
// Defaults (adapt_curve_check): panels = the largest power of two p <= 65536 with M p <= 65536,
// at least 1 (a curve's cells are short already; the sweep's minimum of 16 is for whole
// ranges); max_intervals = max_total / M. The capacity is dealt to the cells in equal parts: a
// singular point inside a very fine grid caps its own cell.
// Left out: parameter rows of curves, a cap shared between cells, infinite ends, the partition,
// more than one rank.
// ---------------------------------------------------------------------------------------
constexpr uint64_t kAdaptCurveMaxCells = 1ull << 20;

struct AdaptCurveResult {
  // per point, M + 1 entries; entry 0 is 0 (converged)
  std::vector<double> x, value, err_est, tol, resabs;
  std::vector<uint8_t> converged;
  AdaptSweepResult cells;      // per cell, M rows
  std::vector<double> atol_cell;  // atol_c
  double total = 0.0, total_err_est = 0.0, total_tol = 0.0, total_resabs = 0.0;
  uint64_t unconverged = 0;    // cells
  uint64_t call_rounds = 0, call_evals = 0, peak = 0;
  double device_ms = 0.0;      // the rounds and the prefix kernel
  uint64_t points() const { return value.size(); }
};

// The options resolved (panels, max_intervals) after every refusal, no device needed: the grid
// (2..2^20 + 1 finite points, strictly monotone, the first offending index named, a finite
// x_M - x_0), `unbounded`, then adapt_sweep_ranges_check's on the resolved options.
AdaptSweepOptions adapt_curve_check(const std::vector<double>& x, const AdaptSweepOptions& opt);
// atol_c of every cell, in the documented order.
std::vector<double> adapt_curve_atol(const std::vector<double>& x, double atol);

class ExprAdaptiveCurve {
 public:
  ExprAdaptiveCurve(const std::string& expr, int device = 0);
  ExprAdaptiveCurve(const ExprAdaptiveCurve&) = delete;
  ExprAdaptiveCurve& operator=(const ExprAdaptiveCurve&) = delete;
  AdaptCurveResult integrate(const std::vector<double>& x, const AdaptSweepOptions& opt = {});
  // Device ms of miint_acurve_prefix alone over `iters` launches on a state of `cells` zero
  // cells (what the kernel costs does not depend on the values).
  double time_prefix(uint64_t cells, int iters);
  const std::string& expression() const { return sweep_.expression(); }

 private:
  ExprAdaptiveSweep sweep_;
};

// ---------------------------------------------------------------------------------------
// Integrals over a box in up to 16 variables: f(x0, ..., x{d-1}) on [a_0, b_0] x ... by a
// randomly shifted rank-1 lattice rule, with an error estimate from the shifts.
//
// The tensor route ends at two variables (ExprIntegrator2D needs 2^30 samples for a 32768^2
// rule). Here n = 2^m points serve any d <= 16. With a generating vector z (d odd entries below
// n), point i of shift r has in dimension j the 32-bit fixed-point fraction
//   u = (((i z_j) mod n) << (32 - m)) + shift[r][j]   (mod 2^32)
// and, by default, the tent transform of it, which makes a smooth non-periodic integrand
// converge like a periodic one:
//   s = (int32)u >> 31, w = (u ^ s) & 0x7FFFFFFF, t = fma((double)w, 2^-31, 2^-32)
// exactly 1 - |2 tau - 1| of the centred fraction tau = (u + 1/2) / 2^32. `periodic` skips the
// tent: t = fma((double)u, 2^-32, 2^-33). Either way t lies strictly inside (0, 1), so no face
// of the box is evaluated, and x_j = fma(t, b_j - a_j, a_j) with b_j - a_j rounded once on the
// host. Every t is a dyadic rational, so piecewise-linear and indicator integrands on boxes of
// power-of-two widths sum exactly in fp64. shift[r][j] is the high 32 bits of splitmix64 at
// the counter r * 16 + j (lattice_shifts), or the caller's own R x d words.
//   est_r = (vol * scale) * S_r / n, S_r the sum of f over the n points of shift r
//   value = (sum est_r) / R in index order
//   err_est = sqrt(sum (est_r - value)^2 / (R (R - 1))): one standard error, not a bound;
//             +inf for R = 1
// Three kernels (expr_lattice.cpp), compiled per (expression, d, periodic):
//
//   miint_lattice_partials  grid (gx, gy): gx point slices x gy shift lanes. A lane walks a
//                           contiguous run of point indices (the prelude's balanced split). At
//                           its first point it forms each u_j from the 64-bit product i0 z_j;
//                           after that a sample costs per dimension one wrapping 32-bit add of
//                           the uniform step z_j << (32 - m) (the wrap is the mod n), the tent's
//                           shift, xor and and, one conversion and two fma; then f and one add
//                           into one of four accumulators. One partial per (shift, bx)
//   miint_lattice_close     per shift, the closing step over its gx partials -> S_r
//   (world > 1)             all-reduce of the R sums
//   miint_lattice_finish    one workgroup: est_r, value, err_est in the order above, stored to
//                           pinned host memory
//
// gx depends on the slice's point count (and an explicit grid) only, never on R, so shift r's
// estimate is bitwise the same alone, among 17 shifts and at any position. No workgroup waits
// on another and every sum has a fixed order: bitwise reproducible. a_j > b_j negates the
// volume; a_j == b_j gives 0 with no launch.
//
// Generating vectors are of Korobov form, z_j = a^j mod n, one built-in a for each m of
// kLatticeBuiltinMin..kLatticeBuiltinMax, chosen by tools/lattice_search.py; for another m, or
// on request, the caller passes z. integrate_to walks m upwards, each level a fresh rule with
// the same shifts, to the first level with err_est <= max(atol, rtol |value|).
// ---------------------------------------------------------------------------------------
constexpr int kLatticeMaxDim = 16;
constexpr int kLatticeMinM = 2, kLatticeMaxM = 30;
constexpr int kLatticeMaxShifts = 4096;
constexpr int kLatticeBuiltinMin = 10, kLatticeBuiltinMax = 26;
constexpr int kLatticeMaxGrid = 2048;  // gx, and about gx * gy
// Least points per lane worth one more workgroup along the points (ExprSweep's measured 256).
constexpr uint64_t kLatticeMinPointsPerLane = 256;

// The sides of the box: (a_j, b_j) for j < d.
using LatticeBox = std::vector<std::pair<double, double>>;

struct LatticeOptions {
  int shifts = 16;                    // R, when shift_words is empty
  uint64_t seed = 0;                  // of lattice_shifts
  std::vector<uint32_t> shift_words;  // R x d explicit shift words, row-major (R from the size)
  std::vector<uint64_t> z;            // d entries; empty: the built-in vector of m
  double rtol = 0.0, atol = 0.0;      // integrate_to only
  int m_min = 12;                     // integrate_to: the first level
  int m_max = 0;                      // integrate_to: the last one; 0 or above the built-in
                                      // range: kLatticeBuiltinMax
};
struct LatticeResult {
  double value = 0.0, err_est = 0.0;
  std::vector<double> estimates;  // est_r
  int m = 0;                      // the (last) level
  uint64_t n = 0;                 // 2^m
  int shifts = 0;                 // R
  uint64_t evals = 0;  // integrate: R x count of this call's slice; integrate_to: R x n, all levels
  int levels = 1;
  bool converged = false;  // integrate_to: the tolerance was met; integrate asks none: false
  double device_ms = 0.0;  // events around the call's kernels (and collectives)
};

// The built-in Korobov vector z_j = a^j mod 2^m, j < d. Throws, naming m, outside the table.
std::vector<uint64_t> lattice_generator(int m, int d);
// The table's multiplier a of m (tools/lattice_search.py prints it).
uint64_t lattice_multiplier(int m);
// shift[r][j], row-major R x d: the high 32 bits of splitmix64 at counter q = r * 16 + j:
// z = seed + (q + 1) 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
// z = (z ^ z >> 27) 0x94D049BB133111EB; z ^= z >> 31.
std::vector<uint32_t> lattice_shifts(uint64_t seed, int shifts, int d);
// Throws, naming the numbers, unless 1 <= d <= 16, 2 <= m <= 30, the box and the scale are
// finite (the widths too), 1 <= R <= 4096 (shift_words a multiple of d), every given z_j is
// odd and below n (or m has a built-in vector) and [begin, begin + count) lies in [0, n). No
// device needed; nothing is launched after a refusal.
void lattice_check(const LatticeBox& box, int m, const LatticeOptions& opt, uint64_t begin,
                   uint64_t count, double scale = 1.0);
// The same for integrate_to: rtol and atol finite, >= 0 and not both 0, m_min <= the clamped
// m_max, both in the built-in range, no explicit z.
void lattice_check_walk(const LatticeBox& box, const LatticeOptions& opt, double scale = 1.0);
struct LatticeShape {
  int gx = 1, gy = 1;
};
// Launch shape for `count` points and R shifts (no device needed): gx = grid if given, else
// clamp(ceil(count / (256 * kLatticeMinPointsPerLane)), 1, 2048); gy = clamp(2048 / gx, 1, R).
LatticeShape lattice_shape(uint64_t count, int shifts, int grid = 0);
// Kernel source for f(x0..x{d-1}); an xJ at or above d fails in the compiler.
std::string expr_lattice_source(const std::string& expr, int d, bool periodic = false);
// hipRTC compile for gfx950 (no device needed), cached per (expression, d, periodic).
std::string expr_lattice_compile(const std::string& expr, int d, bool periodic = false);

class ExprLattice {
 public:
  ExprLattice(const std::string& expr, int d, bool periodic = false, int device = 0,
              int grid = 0);
  ExprLattice(const ExprLattice&) = delete;
  ExprLattice& operator=(const ExprLattice&) = delete;
  // The rule of level m on points [begin, begin + count) of its n = 2^m. With a communicator
  // of more than one rank the ranks' sums S_r are all-reduced between close and finish, so
  // every rank gets the whole rule's result. Synchronous.
  LatticeResult integrate(const LatticeBox& box, int m, const LatticeOptions& opt = {},
                          uint64_t begin = 0, uint64_t count = ~0ull, double scale = 1.0,
                          const Comm* comm = nullptr);
  // The walk over m described above; with a communicator every level's points are split by
  // rank_slice over its ranks. result.levels and result.evals count every level, the other
  // fields are the last level's.
  LatticeResult integrate_to(const LatticeBox& box, const LatticeOptions& opt, double scale = 1.0,
                             const Comm* comm = nullptr);
  // Device ms per integrate() of one rank over `iters` back-to-back ones (shifts uploaded once,
  // before the clock). Hooks as in ExprIntegrator::time.
  double time(const LatticeBox& box, int m, const LatticeOptions& opt, uint64_t begin,
              uint64_t count, int iters, const std::function<void()>& at_start = {},
              const std::function<void()>& at_end = {});
  // Partials go to the caller's device memory (`capacity` doubles) instead of the object's
  // own buffer; a call whose R x gx partials would not fit is refused up front. nullptr: back
  // to the object's buffer.
  void use_partials(double* device_ptr, uint64_t capacity);
  const std::string& expression() const { return expr_; }
  int dim() const { return d_; }
  bool periodic() const { return periodic_; }

 private:
  struct Plan;
  Plan plan(const LatticeBox& box, int m, const LatticeOptions& opt, uint64_t begin,
            uint64_t count, double scale) const;
  void upload(const Plan& p, hipStream_t s);
  void enqueue(const Plan& p, const Comm* comm, hipStream_t s);
  std::string expr_;
  int d_;
  bool periodic_;
  int device_, grid_;
  Stream stream_;
  DeviceBuffer<unsigned> shifts_;
  DeviceBuffer<double> partials_, sums_;
  double* user_partials_ = nullptr;
  uint64_t user_capacity_ = 0;
  PinnedBuffer<unsigned> host_shifts_;
  PinnedBuffer<double> host_out_;  // [0] value, [1] err_est, [2 + r] est_r
  Event e0_, e1_;
  detail::RtcModule module_;  // the last member: destroyed first (miint/expr_rtc.hpp)
};

}  // namespace miint
