// Parameter sweeps of a runtime integrand: f(x, p0..p7) over K rows per launch (see
// miint/expr.hpp, ExprSweep).
#include <algorithm>
#include <cmath>
#include <fstream>
#include <sstream>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kSweepBlock = 256;
enum { kPartials, kClose };  // module_'s kernels

int checked_nparams(int nparams) {
  MIINT_CHECK(nparams >= 0 && nparams <= kSweepMaxParams,
              "expression sweep: nparams must be 0.." + std::to_string(kSweepMaxParams));
  return nparams;
}
int checked_grid(int grid) {
  MIINT_CHECK(grid >= 0 && grid <= kSweepMaxGrid, "expression sweep: grid must be 0 (auto) ..2048");
  return grid;
}
}  // namespace

std::string expr_sweep_source(const std::string& expr, int nparams) {
  expr_check(expr);
  checked_nparams(nparams);
  std::string sig, load, args;  // ", double p0, ..." / "const double p0 = pr[0]; ..." / ", p0, ..."
  for (int j = 0; j < nparams; ++j) {
    const std::string p = "p" + std::to_string(j);
    sig += ", double " + p;
    load += "    const double " + p + " = pr[" + std::to_string(j) + "];\n";
    args += ", " + p;
  }
  return std::string(detail::kRtcPrelude) + R"(
__device__ __forceinline__ double miint_fp(double x)" + sig + R"() { return ()" + expr + R"(); }
#define MIINT_AT(idx) miint_fp(fma(idx, h, av))" + args + R"()

// K parameter rows in one launch. gridDim.x sample slices x gridDim.y row lanes: workgroup
// (bx, by) walks rows k0 + by, k0 + by + gridDim.y, ... below k0 + kc. A row's parameters are
// workgroup-uniform reads of params[k * nparams + j] (never written here). Per row the
// per-sample loop is miint_expr_partials's: the lane's share (miint_lane_share) through
// MIINT_SAMPLE_SUM, then the block sum. One partial per (row, bx) at
// partials[(k - k0) * gridDim.x + bx]. The per-lane count is 32-bit: the host refuses a
// shape whose lanes would take 2^32 samples or more (expr_sweep_shape). No workgroup waits
// on another: rows are independent and the close is a kernel of its own.
extern "C" __global__ __launch_bounds__(256) void miint_expr_sweep_partials(
    double a, double h, double off, unsigned long long i0, unsigned long long n,
    const double* __restrict__ params, int nparams, unsigned k0, unsigned kc,
    double* __restrict__ partials) {
  __shared__ double red[2][4];  // alternating per row: one barrier per row is enough
  unsigned long long start;
  const unsigned cnt = miint_lane_share(n, &start);
  const double idx0 = (double)(i0 + start) + off;
  // a in a vector register for the whole kernel: an fma takes one scalar operand (h), and
  // inside the row loop the compiler otherwise copies a from its scalar register in every
  // iteration of the sample loop (1 VALU in 67 for 4/(1+p0 x^2), 1.2 % of a row's time;
  // miint_expr_partials gets the VGPR copy hoisted by itself)
  double av = a;
  asm("" : "+v"(av));
  unsigned par = 0;
  for (unsigned k = k0 + blockIdx.y; k < k0 + kc; k += gridDim.y, par ^= 1u) {
    const double* __restrict__ pr = params + (unsigned long long)k * (unsigned)nparams;
    (void)pr;
)" + load + R"(    MIINT_SAMPLE_SUM(acc, idx0, cnt, MIINT_AT);
    MIINT_BLOCK_SUM(acc, red[par]);
    if (threadIdx.x == 0)
      partials[(unsigned long long)(k - k0) * gridDim.x + blockIdx.x] = MIINT_RED(red[par]);
  }
}

// One workgroup per row of the chunk closes the row's gx partials: out[k] = scale * sum.
extern "C" __global__ __launch_bounds__(256) void miint_expr_sweep_close(
    const double* __restrict__ partials, int gx, unsigned kc, double scale,
    double* __restrict__ out) {
  const unsigned k = blockIdx.x;
  if (k >= kc) return;
  const double* row = partials + (unsigned long long)k * (unsigned)gx;
  MIINT_CLOSE(row, gx, scale, out[k]);
}
)";
}

std::string expr_sweep_compile(const std::string& expr, int nparams) {
  return detail::rtc_compile_cached(expr_sweep_source(expr, nparams), expr);
}

SweepShape expr_sweep_shape(uint64_t n_local, uint64_t rows, int grid) {
  MIINT_CHECK(rows >= 1 && rows <= kSweepMaxRows, "expression sweep: rows must be 1..2^20");
  checked_grid(grid);
  SweepShape s;
  if (grid > 0) {
    s.gx = grid;
  } else {
    const uint64_t per_wg = kSweepBlock * kSweepMinSamplesPerLane;
    const uint64_t want = n_local / per_wg + (n_local % per_wg ? 1 : 0);
    s.gx = static_cast<int>(std::min<uint64_t>(std::max<uint64_t>(want, 1), kSweepMaxGrid));
  }
  s.gy = static_cast<int>(
      std::min<uint64_t>(std::max<uint64_t>(kSweepMaxGrid / s.gx, 1), rows));
  detail::check_lane_count("expression sweep", n_local,
                           static_cast<uint64_t>(s.gx) * kSweepBlock);
  return s;
}

std::vector<double> load_param_rows(const std::string& path, int* nparams) {
  std::ifstream in(path);
  MIINT_CHECK(in.good(), "cannot read parameter file " + path);
  std::vector<double> v;
  std::string line;
  int lineno = 0, width = -1;
  uint64_t rows = 0;
  while (std::getline(in, line)) {
    ++lineno;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    for (char& c : line)
      if (c == ',' || c == ';' || c == '\t' || c == '\r') c = ' ';
    std::istringstream ls(line);
    std::string tok;
    int w = 0;
    const std::string where = path + ":" + std::to_string(lineno) + ": row " + std::to_string(rows);
    while (ls >> tok) {
      char* end = nullptr;
      const double x = std::strtod(tok.c_str(), &end);
      MIINT_CHECK(end && *end == '\0' && std::isfinite(x),
                  where + ": not a finite number: '" + tok + "'");
      v.push_back(x);
      ++w;
    }
    if (w == 0) continue;  // blank or comment
    if (width < 0) width = w;
    MIINT_CHECK(w == width, where + " has " + std::to_string(w) + " values, row 0 has " +
                                std::to_string(width));
    MIINT_CHECK(w <= kSweepMaxParams, where + ": at most 8 parameters per row");
    ++rows;
    MIINT_CHECK(rows <= kSweepMaxRows, where + ": at most 2^20 rows");
  }
  MIINT_CHECK(rows >= 1, path + ": no parameter rows (row 0 is missing)");
  *nparams = width;
  return v;
}

std::vector<double> linspace_param_rows(const std::string& spec) {
  const std::string want = "--linspace wants p0=LO:HI:COUNT (got '" + spec + "')";
  MIINT_CHECK(spec.rfind("p0=", 0) == 0, want);
  const char* s = spec.c_str() + 3;
  char* end = nullptr;
  const double lo = std::strtod(s, &end);
  MIINT_CHECK(end != s && *end == ':', want);
  s = end + 1;
  const double hi = std::strtod(s, &end);
  MIINT_CHECK(end != s && *end == ':', want);
  s = end + 1;
  const double cnt = std::strtod(s, &end);
  MIINT_CHECK(end != s && *end == '\0' && cnt >= 1 && cnt <= static_cast<double>(kSweepMaxRows) &&
                  cnt == std::floor(cnt) && std::isfinite(lo) && std::isfinite(hi),
              want);
  const uint64_t k = static_cast<uint64_t>(cnt);
  std::vector<double> v(k);
  for (uint64_t i = 0; i < k; ++i)
    v[i] = k == 1 ? lo : (i + 1 == k ? hi : lo + (hi - lo) * (static_cast<double>(i) / (k - 1)));
  return v;
}

ExprSweep::ExprSweep(const std::string& expr, int nparams, int device, int grid)
    : expr_(expr), nparams_(checked_nparams(nparams)), device_(device), grid_(checked_grid(grid)),
      stream_((set_device(device), Stream())),
      module_(expr_sweep_compile(expr, nparams), device, stream_,
              {"miint_expr_sweep_partials", "miint_expr_sweep_close"}) {}

void ExprSweep::check(const std::vector<double>& params, uint64_t rows, uint64_t n,
                      uint64_t begin, uint64_t count) const {
  MIINT_CHECK(rows <= kSweepMaxRows, "expression sweep: at most 2^20 rows");
  MIINT_CHECK(params.size() == rows * static_cast<uint64_t>(nparams_),
              "expression sweep: " + std::to_string(params.size()) + " parameter values for " +
                  std::to_string(rows) + " rows of " + std::to_string(nparams_));
  for (double p : params) MIINT_CHECK(std::isfinite(p), "expression sweep: non-finite parameter");
  detail::check_slice("expression sweep", n, begin, count);
}

// Buffers grow to the largest sweep seen (at least one element each); then the rows go to
// the device through pinned memory.
void ExprSweep::upload(const std::vector<double>& params, uint64_t rows, int gx, hipStream_t s) {
  const size_t np = std::max<size_t>(params.size(), 1);
  if (params_.size() < np) {
    params_ = DeviceBuffer<double>(np);
    host_params_ = PinnedBuffer<double>(np);
  }
  if (out_.size() < rows) {
    out_ = DeviceBuffer<double>(rows);
    host_out_ = PinnedBuffer<double>(rows);
  }
  const uint64_t chunk = std::min<uint64_t>(rows, std::max<uint64_t>(kSweepMaxPartials / gx, 1));
  if (partials_.size() < chunk * gx) partials_ = DeviceBuffer<double>(chunk * gx);
  if (!params.empty()) {
    std::copy(params.begin(), params.end(), host_params_.get());
    MIINT_HIP(hipMemcpyAsync(params_.get(), host_params_.get(), params.size() * sizeof(double),
                             hipMemcpyHostToDevice, s));
  }
}

void ExprSweep::enqueue(double a, double h, double off, uint64_t begin, uint64_t count,
                        uint64_t rows, SweepShape shape, double scale, hipStream_t s) {
  const int gx = shape.gx;
  const uint64_t chunk = std::min<uint64_t>(rows, std::max<uint64_t>(kSweepMaxPartials / gx, 1));
  for (uint64_t r0 = 0; r0 < rows; r0 += chunk) {
    const unsigned k0 = static_cast<unsigned>(r0);
    const unsigned kc = static_cast<unsigned>(std::min<uint64_t>(chunk, rows - r0));
    const unsigned gy = std::min<unsigned>(static_cast<unsigned>(shape.gy), kc);
    module_.launch(kPartials, gx, gy, kSweepBlock, s, a, h, off, begin, count, params_.get(),
                   nparams_, k0, kc, partials_.get());
    module_.launch(kClose, kc, 1, kSweepBlock, s, partials_.get(), gx, kc, scale,
                   out_.get() + r0);
  }
}

std::vector<double> ExprSweep::integrate(const std::vector<double>& params, uint64_t rows,
                                         double a, double b, uint64_t n, Rule rule,
                                         uint64_t begin, uint64_t count, double scale,
                                         const Comm* comm) {
  check(params, rows, n, begin, count);
  if (rows == 0) return {};
  const SweepShape shape = expr_sweep_shape(count, rows, grid_);
  DeviceGuard g(device_);
  const double h = (b - a) / static_cast<double>(n);
  hipStream_t s = stream_.get();
  upload(params, rows, shape.gx, s);
  enqueue(a, h, rule_offset(rule), begin, count, rows, shape, h * scale, s);
  if (comm && comm->world() > 1) comm->allreduce_sum(out_.get(), out_.get(), rows, s);
  MIINT_HIP(hipMemcpyAsync(host_out_.get(), out_.get(), rows * sizeof(double),
                           hipMemcpyDeviceToHost, s));
  stream_.sync();
  return std::vector<double>(host_out_.get(), host_out_.get() + rows);
}

double ExprSweep::time(const std::vector<double>& params, uint64_t rows, double a, double b,
                       uint64_t n, Rule rule, uint64_t begin, uint64_t count, int iters,
                       const std::function<void()>& at_start,
                       const std::function<void()>& at_end) {
  check(params, rows, n, begin, count);
  MIINT_CHECK(iters >= 1 && rows >= 1, "bad expression sweep timing request");
  const SweepShape shape = expr_sweep_shape(count, rows, grid_);
  DeviceGuard g(device_);
  const double h = (b - a) / static_cast<double>(n);
  hipStream_t s = stream_.get();
  upload(params, rows, shape.gx, s);
  return detail::time_enqueues(
      stream_, e0_, e1_, iters,
      [&] { enqueue(a, h, rule_offset(rule), begin, count, rows, shape, h, s); }, at_start,
      at_end);
}

}  // namespace miint
