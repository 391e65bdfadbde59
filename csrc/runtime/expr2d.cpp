// Double integrals of a runtime integrand: f(x, y) over a rectangle (see miint/expr.hpp,
// ExprIntegrator2D).
#include <algorithm>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kExpr2DBlock = 256;
enum { kPartials, kFinalize };  // module_'s kernels

int checked_grid(int grid) {
  MIINT_CHECK(grid >= 0 && grid <= kExpr2DMaxGrid,
              "expression 2-D: grid must be 0 (auto) ..2048");
  return grid;
}
using u128 = unsigned __int128;

uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b ? 1 : 0); }
}  // namespace

namespace detail {
// expr_check names the character or word it refuses; here the expression is named too.
void expr_check_named(const std::string& expr) {
  try {
    expr_check(expr);
  } catch (const std::exception& e) {
    fail("expression '" + expr + "' is rejected: " + e.what(), __FILE__, __LINE__);
  }
}
}  // namespace detail

std::string expr2d_source(const std::string& expr) {
  detail::expr_check_named(expr);
  return std::string(detail::kRtcPrelude) + R"(
__device__ __forceinline__ double miint_f2(double x, double y) {
  (void)x; (void)y;
  return ()" + expr + R"();
}

// `cnt` rows down NV fixed columns: y once per row and shared by the columns, so a sample
// costs f and one add; whatever f does with x alone is loop-invariant and leaves the loop.
// The row index is an exact fp64 (j += 1, exact below 2^52), as in miint_expr_partials.
template <int NV>
__device__ __forceinline__ void miint_rows(const double (&x)[4], double j, double hy, double ay,
                                           unsigned cnt, double (&acc)[4]) {
  for (unsigned k = 0; k < cnt; ++k) {
    const double y = fma(j, hy, ay);
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] += miint_f2(x[c], y);
    j += 1.0;
  }
}

// The 256 lanes are lx lanes along x by 256 / lx lanes along y (lx = 1 << lx_log2). An item
// is one column panel (lx * cpl columns) by one row stretch; the rows are dealt to the
// `stretches` stretches in balanced contiguous runs, a stretch's rows to the lanes along y
// likewise. Lane (tx, ty) owns columns panel * lx * cpl + c * lx + tx, c < cpl (those below
// nx: a prefix of them), forms their x once per item and runs down its rows. Workgroup w
// takes items [w * ipw, min((w + 1) * ipw, items)), item = panel * stretches + stretch, and
// keeps its four accumulators across them; wave64 butterfly, four waves through LDS, one
// partial per workgroup. The host (expr2d_shape / expr2d_check) keeps cpl in 1..4, a lane's
// rows of a stretch and ipw below 2^32. No workgroup waits on another. No occupancy bound is
// asked for: for 4/(1+x*x+y*y) 8 waves a SIMD (62 VGPRs instead of 72) measured 1.6 % slower,
// and a heavier f (exp(-x*x)*cos(x*y)) would spill under it (profiles/r16/expr2d.md).
extern "C" __global__ __launch_bounds__(256) void miint_expr2d_partials(
    double ax, double hx, double ay, double hy, double off, unsigned long long nx,
    unsigned long long row0, unsigned long long rows, unsigned lx_log2, unsigned cpl,
    unsigned long long stretches, unsigned long long items, unsigned long long ipw,
    double* __restrict__ partials) {
  __shared__ double red[4];
  const unsigned lx = 1u << lx_log2, ly = 256u >> lx_log2;
  const unsigned tx = threadIdx.x & (lx - 1u), ty = threadIdx.x >> lx_log2;
  const unsigned long long sq = rows / stretches, sr = rows % stretches;
  const unsigned long long first = (unsigned long long)blockIdx.x * ipw;
  const unsigned long long last = first + ipw < items ? first + ipw : items;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned long long panel = first / stretches, st = first % stretches;  // one division
  for (unsigned long long it = first; it < last; ++it) {
    const unsigned long long c0 = panel * ((unsigned long long)lx * cpl) + tx;
    double x[4];
    unsigned nv = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned long long col = c0 + (unsigned long long)c * lx;
      nv += ((unsigned)c < cpl && col < nx) ? 1u : 0u;
      x[c] = fma((double)col + off, hx, ax);
    }
    const unsigned long long sb = st * sq + (st < sr ? st : sr);   // the stretch's rows
    const unsigned long long sc = sq + (st < sr ? 1ull : 0ull);
    const unsigned long long lq = sc >> (8u - lx_log2), lr = sc & (ly - 1u);  // the lane's share
    const unsigned long long lb = (unsigned long long)ty * lq + (ty < lr ? ty : lr);
    const unsigned cnt = (unsigned)(lq + (ty < lr ? 1ull : 0ull));
    const double j = (double)(row0 + sb + lb) + off;
    switch (nv) {
      case 4: miint_rows<4>(x, j, hy, ay, cnt, acc); break;
      case 3: miint_rows<3>(x, j, hy, ay, cnt, acc); break;
      case 2: miint_rows<2>(x, j, hy, ay, cnt, acc); break;
      case 1: miint_rows<1>(x, j, hy, ay, cnt, acc); break;
      default: break;
    }
    if (++st == stretches) {  // the next item: the next stretch, or the next panel's first
      st = 0;
      ++panel;
    }
  }
  double v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  MIINT_BLOCK_SUM(v, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = MIINT_RED(red);
}

// scale is (hx * hy) * the caller's scale, applied once.
extern "C" __global__ __launch_bounds__(256) void miint_expr2d_finalize(
    const double* __restrict__ partials, int n, double scale, double* __restrict__ out) {
  MIINT_CLOSE(partials, n, scale, out[0]);
}
)";
}

std::string expr2d_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr2d_source(expr), expr);
}

// Every (lanes along x, columns per lane, rows per lane) candidate is priced by what the
// launch would dispatch, and the cheapest of those that fill their slots wins:
//   slots = workgroups * 256 * (columns per lane * rows per lane * items per workgroup)
//   fill  = nx * row_count / slots
//   cost  = max(per-lane samples, 64) * max(workgroups, 512)
//           * (1 + 0.05 (4 - cpl)) * (1 + 2 / rows per lane)
// The cost is a guess at the time, and its weights (64 samples, 512 workgroups, 5 % per
// missing column, 2 / rows) are not measured: the longest lane sets the time once the device
// is full; under about 2 waves a SIMD (512 workgroups) the lanes' latency shows; under 64
// samples a lane costs its set-up and the reduction; fewer columns mean less ILP and less
// sharing of y; short row runs pay for x and the loop set-up more often. Only the shapes it
// chooses for 32768^2 and the two skinny 2^30-sample rules were timed
// (profiles/r16/expr2d.md). Not all 2048 workgroups need be resident at once: at 72 VGPRs
// (4/(1+x*x+y*y)) 1536 are, and the rest follow as those retire.
// Only candidates with fill >= 3/4 of the best fill compete, so the chosen shape keeps
// more than half of its slots busy wherever some candidate fills 2/3 (the CPU test sweeps
// it). Ties go to the first candidate in (lx, cpl, rows) order: a pure function of
// (nx, row_count, grid).
Expr2DShape expr2d_shape(uint64_t nx, uint64_t row_count, int grid) {
  detail::check_2d_nx("expression 2-D", nx);
  MIINT_CHECK(row_count >= 1 && row_count <= kExpr2DMaxNy,
              "expression 2-D: " + std::to_string(row_count) + " rows must be 1..2^40");
  checked_grid(grid);
  const uint64_t cap = grid > 0 ? static_cast<uint64_t>(grid) : kExpr2DMaxGrid;
  static const uint64_t kRows[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256};
  const long double total = static_cast<long double>(nx) * static_cast<long double>(row_count);
  struct Cand {
    Expr2DShape s;
    long double fill = 0, cost = 0;
  };
  std::vector<Cand> cands;
  long double best_fill = 0;
  for (int lg = 0; lg <= 8; ++lg) {
    const uint64_t lx = 1ull << lg, ly = kExpr2DBlock / lx;
    for (uint64_t cpl = 1; cpl <= 4; ++cpl) {
      const uint64_t panels = ceil_div(nx, lx * cpl);
      uint64_t prev = 0;
      for (uint64_t want : kRows) {
        // `want` rows per lane asks for this many stretches; the rows are then dealt evenly
        const uint64_t stretches = std::max<uint64_t>(ceil_div(row_count, ly * want), 1);
        const uint64_t rpl = ceil_div(ceil_div(row_count, stretches), ly);
        if (rpl == prev) continue;
        prev = rpl;
        const u128 items = static_cast<u128>(panels) * stretches;
        const u128 ipw = (items + cap - 1) / cap;
        const u128 wgs = (items + ipw - 1) / ipw;
        const u128 per_lane = static_cast<u128>(cpl * rpl) * ipw;
        if (ipw >> 32 || per_lane >> 32) continue;  // the kernel's 32-bit counts
        Cand c;
        c.s.lanes_x = static_cast<int>(lx);
        c.s.cols_per_lane = static_cast<int>(cpl);
        c.s.rows_per_item = ceil_div(row_count, stretches);
        c.s.stretches = stretches;
        c.s.panels = panels;
        c.s.items = static_cast<uint64_t>(items);
        c.s.items_per_wg = static_cast<uint64_t>(ipw);
        c.s.workgroups = static_cast<int>(wgs);
        c.s.lane_samples = static_cast<uint64_t>(per_lane);
        const long double slots =
            static_cast<long double>(wgs) * kExpr2DBlock * static_cast<long double>(per_lane);
        c.fill = total / slots;
        c.cost = std::max<long double>(static_cast<long double>(per_lane), 64.0L) *
                 std::max<long double>(static_cast<long double>(wgs), 512.0L) *
                 (1.0L + 0.05L * (4 - static_cast<int>(cpl))) * (1.0L + 2.0L / rpl);
        best_fill = std::max(best_fill, c.fill);
        cands.push_back(c);
      }
    }
  }
  MIINT_CHECK(!cands.empty(),
              "expression 2-D: " + std::to_string(nx) + " x " + std::to_string(row_count) +
                  " samples over " + std::to_string(cap) + " workgroups pass the 32-bit "
                  "per-lane count; use a larger grid or fewer rows per launch");
  const Cand* best = nullptr;
  for (const Cand& c : cands)
    if (c.fill >= 0.75L * best_fill && (!best || c.cost < best->cost)) best = &c;
  return best->s;
}

Expr2DShape expr2d_plan(uint64_t nx, uint64_t ny, uint64_t row_begin, uint64_t row_count,
                        int grid) {
  detail::check_2d_range("expression 2-D", nx, ny, row_begin, row_count);
  if (row_count == 0) {  // nothing to launch
    Expr2DShape none;
    none.rows_per_item = none.stretches = none.panels = none.items = none.items_per_wg = 0;
    none.workgroups = 0;
    none.lane_samples = 0;
    return none;
  }
  return expr2d_shape(nx, row_count, grid);  // refuses an over-full lane; never sees row_begin
}

void expr2d_check(uint64_t nx, uint64_t ny, uint64_t row_begin, uint64_t row_count, int grid) {
  (void)expr2d_plan(nx, ny, row_begin, row_count, grid);
}

ExprIntegrator2D::ExprIntegrator2D(const std::string& expr, int device, int grid)
    : expr_(expr), device_(device), grid_(checked_grid(grid)),
      stream_((set_device(device), Stream())),
      module_(expr2d_compile(expr), device, stream_,
              {"miint_expr2d_partials", "miint_expr2d_finalize"}) {
  DeviceGuard g(device);
  partials_ = DeviceBuffer<double>(static_cast<size_t>(kExpr2DMaxGrid));
  out_ = DeviceBuffer<double>(1);
  host_ = PinnedBuffer<double>(1);
}

// row_count == 0 (a rank beyond ny): no kernel, the value is 0.0. `sh` is the call's
// expr2d_plan, made once per integrate / time call.
void ExprIntegrator2D::enqueue(const Expr2DShape& sh, double ax, double hx, double ay, double hy,
                               double off, uint64_t nx, uint64_t row_begin, uint64_t row_count,
                               double scale, hipStream_t s) {
  if (row_count == 0) {
    MIINT_HIP(hipMemsetAsync(out_.get(), 0, sizeof(double), s));
    return;
  }
  unsigned lx_log2 = 0;
  while ((1 << lx_log2) < sh.lanes_x) ++lx_log2;
  module_.launch(kPartials, sh.workgroups, 1, kExpr2DBlock, s, ax, hx, ay, hy, off, nx, row_begin,
                 row_count, lx_log2, static_cast<unsigned>(sh.cols_per_lane), sh.stretches,
                 sh.items, sh.items_per_wg, partials_.get());
  module_.launch(kFinalize, 1, 1, kExpr2DBlock, s, partials_.get(), sh.workgroups, scale,
                 out_.get());
}

double ExprIntegrator2D::integrate(double ax, double bx, uint64_t nx, double ay, double by,
                                   uint64_t ny, Rule rule, uint64_t row_begin,
                                   uint64_t row_count, double scale, const Comm* comm) {
  const Expr2DShape sh = expr2d_plan(nx, ny, row_begin, row_count, grid_);
  DeviceGuard g(device_);
  const double hx = (bx - ax) / static_cast<double>(nx);
  const double hy = (by - ay) / static_cast<double>(ny);
  hipStream_t s = stream_.get();
  enqueue(sh, ax, hx, ay, hy, rule_offset(rule), nx, row_begin, row_count, (hx * hy) * scale, s);
  if (comm && comm->world() > 1) comm->allreduce_sum(out_.get(), out_.get(), 1, s);
  MIINT_HIP(hipMemcpyAsync(host_.get(), out_.get(), sizeof(double), hipMemcpyDeviceToHost, s));
  stream_.sync();
  return host_[0];
}

double ExprIntegrator2D::time(double ax, double bx, uint64_t nx, double ay, double by,
                              uint64_t ny, Rule rule, uint64_t row_begin, uint64_t row_count,
                              int iters, const std::function<void()>& at_start,
                              const std::function<void()>& at_end) {
  MIINT_CHECK(iters >= 1, "bad expression 2-D timing request");
  const Expr2DShape sh = expr2d_plan(nx, ny, row_begin, row_count, grid_);
  DeviceGuard g(device_);
  const double hx = (bx - ax) / static_cast<double>(nx);
  const double hy = (by - ay) / static_cast<double>(ny);
  const double off = rule_offset(rule);
  hipStream_t s = stream_.get();
  return detail::time_enqueues(
      stream_, e0_, e1_, iters,
      [&] { enqueue(sh, ax, hx, ay, hy, off, nx, row_begin, row_count, hx * hy, s); }, at_start,
      at_end);
}

}  // namespace miint
