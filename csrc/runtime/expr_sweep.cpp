// Parameter sweeps of a runtime integrand: f(x, p0..p7) over K rows per launch (see
// miint/expr.hpp, ExprSweep).
#include <algorithm>
#include <cmath>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kSweepBlock = 256;

void check_nparams(int nparams) {
  MIINT_CHECK(nparams >= 0 && nparams <= kSweepMaxParams,
              "expression sweep: nparams must be 0.." + std::to_string(kSweepMaxParams));
}
}  // namespace

std::string expr_sweep_source(const std::string& expr, int nparams) {
  expr_check(expr);
  check_nparams(nparams);
  std::string sig, load, args;  // ", double p0, ..." / "const double p0 = pr[0]; ..." / ", p0, ..."
  for (int j = 0; j < nparams; ++j) {
    const std::string p = "p" + std::to_string(j);
    sig += ", double " + p;
    load += "    const double " + p + " = pr[" + std::to_string(j) + "];\n";
    args += ", " + p;
  }
  auto f = [&](const std::string& x) { return "miint_fp(fma(" + x + ", h, av)" + args + ")"; };
  return R"(
__device__ __forceinline__ double miint_fp(double x)" + sig + R"() { return ()" + expr + R"(); }

// K parameter rows in one launch. gridDim.x sample slices x gridDim.y row lanes: workgroup
// (bx, by) walks rows k0 + by, k0 + by + gridDim.y, ... below k0 + kc. A row's parameters are
// workgroup-uniform reads of params[k * nparams + j] (never written here). Per row the
// per-sample loop is miint_expr_partials's: lane g owns a contiguous balanced run of the
// slice, walked with an exact fp64 index (fma(idx, h, a) per sample), four independent
// accumulators, wave64 butterfly, four waves through LDS. One partial per (row, bx) at
// partials[(k - k0) * gridDim.x + bx]. The per-lane count is 32-bit: the host refuses a
// shape whose lanes would take 2^32 samples or more (expr_sweep_shape). No workgroup waits
// on another: rows are independent and the close is a kernel of its own.
extern "C" __global__ __launch_bounds__(256) void miint_expr_sweep_partials(
    double a, double h, double off, unsigned long long i0, unsigned long long n,
    const double* __restrict__ params, int nparams, unsigned k0, unsigned kc,
    double* __restrict__ partials) {
  __shared__ double red[2][4];  // alternating per row: one barrier per row is enough
  const unsigned long long lanes = (unsigned long long)gridDim.x * 256ull;
  const unsigned long long g = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long q = n / lanes, r = n % lanes;
  const unsigned long long start = g * q + (g < r ? g : r);
  const unsigned cnt = (unsigned)(q + (g < r ? 1ull : 0ull));
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
)" + load + R"(    double idx = idx0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    unsigned c = 0;
    for (; c + 4 <= cnt; c += 4) {
      a0 += )" + f("idx") + R"(;
      a1 += )" + f("idx + 1.0") + R"(;
      a2 += )" + f("idx + 2.0") + R"(;
      a3 += )" + f("idx + 3.0") + R"(;
      idx += 4.0;
    }
    for (; c < cnt; ++c) {
      a0 += )" + f("idx") + R"(;
      idx += 1.0;
    }
    double acc = (a0 + a1) + (a2 + a3);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);  // wave64 butterfly
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
      partials[(unsigned long long)(k - k0) * gridDim.x + blockIdx.x] =
          (red[par][0] + red[par][1]) + (red[par][2] + red[par][3]);
  }
}

// One workgroup per row of the chunk: thread t sums the row's partials t, t + 256, ... in
// order; fixed-order tree after. out[k] = scale * sum.
extern "C" __global__ __launch_bounds__(256) void miint_expr_sweep_close(
    const double* __restrict__ partials, int gx, unsigned kc, double scale,
    double* __restrict__ out) {
  __shared__ double red[4];
  const unsigned k = blockIdx.x;
  if (k >= kc) return;
  const double* row = partials + (unsigned long long)k * (unsigned)gx;
  double v = 0.0;
  for (int i = threadIdx.x; i < gx; i += 256) v += row[i];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[k] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}
)";
}

std::string expr_sweep_compile(const std::string& expr, int nparams) {
  static std::mutex mu;
  static std::map<std::pair<std::string, int>, std::string> cache;  // -> code object
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_pair(expr, nparams);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  return cache[key] = detail::rtc_compile(expr_sweep_source(expr, nparams), expr);
}

SweepShape expr_sweep_shape(uint64_t n_local, uint64_t rows, int grid) {
  MIINT_CHECK(rows >= 1 && rows <= kSweepMaxRows, "expression sweep: rows must be 1..2^20");
  MIINT_CHECK(grid >= 0 && grid <= kSweepMaxGrid, "expression sweep: grid must be 0 (auto) ..2048");
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
  const uint64_t lanes = static_cast<uint64_t>(s.gx) * kSweepBlock;
  MIINT_CHECK(n_local / lanes + 1 < (1ull << 32),
              "expression sweep: " + std::to_string(n_local) + " samples over " +
                  std::to_string(lanes) + " lanes pass the 32-bit per-lane count; use a "
                  "larger grid or slice the samples");
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
    : expr_(expr), nparams_(nparams), device_(device), grid_(grid),
      stream_((set_device(device), Stream())) {
  check_nparams(nparams);
  MIINT_CHECK(grid >= 0 && grid <= kSweepMaxGrid, "expression sweep: grid must be 0 (auto) ..2048");
  const std::string code = expr_sweep_compile(expr, nparams);
  DeviceGuard g(device);
  MIINT_HIP(hipModuleLoadData(&module_, code.data()));
  MIINT_HIP(hipModuleGetFunction(&partials_fn_, module_, "miint_expr_sweep_partials"));
  MIINT_HIP(hipModuleGetFunction(&close_fn_, module_, "miint_expr_sweep_close"));
}

ExprSweep::~ExprSweep() {
  if (module_) {
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_.get());
    (void)hipModuleUnload(module_);
  }
}

void ExprSweep::check(const std::vector<double>& params, uint64_t rows, uint64_t n,
                      uint64_t begin, uint64_t count) const {
  MIINT_CHECK(rows <= kSweepMaxRows, "expression sweep: at most 2^20 rows");
  MIINT_CHECK(params.size() == rows * static_cast<uint64_t>(nparams_),
              "expression sweep: " + std::to_string(params.size()) + " parameter values for " +
                  std::to_string(rows) + " rows of " + std::to_string(nparams_));
  for (double p : params) MIINT_CHECK(std::isfinite(p), "expression sweep: non-finite parameter");
  MIINT_CHECK(n >= 1 && begin + count <= n && begin + count >= begin,
              "expression sweep slice outside [0, n)");
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
  unsigned long long i0 = begin, n = count;
  const double* params = params_.get();
  double* parts = partials_.get();
  int np = nparams_, gx = shape.gx;
  double sc = scale;
  const uint64_t chunk = std::min<uint64_t>(rows, std::max<uint64_t>(kSweepMaxPartials / gx, 1));
  for (uint64_t r0 = 0; r0 < rows; r0 += chunk) {
    unsigned k0 = static_cast<unsigned>(r0);
    unsigned kc = static_cast<unsigned>(std::min<uint64_t>(chunk, rows - r0));
    const unsigned gy = std::min<unsigned>(static_cast<unsigned>(shape.gy), kc);
    void* args[] = {&a, &h, &off, &i0, &n, &params, &np, &k0, &kc, &parts};
    MIINT_HIP(hipModuleLaunchKernel(partials_fn_, gx, gy, 1, kSweepBlock, 1, 1, 0, s, args,
                                    nullptr));
    double* out = out_.get() + r0;
    void* cargs[] = {&parts, &gx, &kc, &sc, &out};
    MIINT_HIP(hipModuleLaunchKernel(close_fn_, kc, 1, 1, kSweepBlock, 1, 1, 0, s, cargs,
                                    nullptr));
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
  enqueue(a, h, rule_offset(rule), begin, count, rows, shape, h, s);  // warm
  stream_.sync();
  if (at_start) at_start();
  e0_.record(s);
  for (int i = 0; i < iters; ++i)
    enqueue(a, h, rule_offset(rule), begin, count, rows, shape, h, s);
  if (at_end) at_end();
  e1_.record(s);
  stream_.sync();
  return Event::elapsed_ms(e0_, e1_) / iters;
}

}  // namespace miint
