// Runtime integrands compiled with hipRTC (see miint/expr.hpp).
#include "miint/expr.hpp"

#include <cctype>

#include "miint/expr_rtc.hpp"

namespace miint {

namespace {
constexpr int kExprBlock = 256;
enum { kPartials, kFinalize };  // module_'s kernels

int checked_grid(int grid) {
  MIINT_CHECK(grid >= 1 && grid <= 65535, "expression grid out of range");
  return grid;
}
}  // namespace

// One C++ expression over x: no statements, blocks, asm or literals that could smuggle them.
void expr_check(const std::string& e) {
  MIINT_CHECK(!e.empty() && e.size() <= 4096, "expression must be 1..4096 characters");
  for (char c : e) {
    const bool ok = std::isalnum(static_cast<unsigned char>(c)) ||
                    std::string(" \t_.+-*/%(),?:<>=!&|^~").find(c) != std::string::npos;
    MIINT_CHECK(ok, std::string("expression: character '") + c + "' not allowed (one C++ "
                    "expression over x: no ; { } [ ] # quotes or backslashes)");
  }
  // digraphs spell the characters refused above: <% %> <: :> %: are { } [ ] #
  for (const char* dg : {"<%", "%>", "<:", ":>", "%:"})
    MIINT_CHECK(e.find(dg) == std::string::npos,
                std::string("expression: digraph '") + dg + "' not allowed (it spells a brace, "
                "bracket or #)");
  // identifiers that are not math: asm / volatile / goto / the preprocessor are out
  std::string word;
  auto bad = [](const std::string& w) {
    return w == "asm" || w == "__asm" || w == "__asm__" || w == "volatile" || w == "goto" ||
           w == "__builtin_amdgcn_s_sendmsg" || w.rfind("__builtin_amdgcn", 0) == 0;
  };
  for (size_t i = 0; i <= e.size(); ++i) {
    const char c = i < e.size() ? e[i] : ' ';
    if (std::isalnum(static_cast<unsigned char>(c)) || c == '_') {
      word += c;
    } else {
      MIINT_CHECK(!bad(word), "expression: '" + word + "' is not allowed");
      word.clear();
    }
  }
}

std::string expr_source(const std::string& expr) {
  expr_check(expr);
  return std::string(detail::kRtcPrelude) + R"(
__device__ __forceinline__ double miint_f(double x) { return ()" + expr + R"(); }
#define MIINT_AT(idx) miint_f(fma(idx, h, a))

// Every sample on its own: each lane's share (miint_lane_share) through MIINT_SAMPLE_SUM,
// then one partial per workgroup.
extern "C" __global__ __launch_bounds__(256) void miint_expr_partials(
    double a, double h, double off, unsigned long long i0, unsigned long long n,
    double* partials) {
  __shared__ double red[4];
  unsigned long long start;
  const unsigned cnt = miint_lane_share(n, &start);
  MIINT_SAMPLE_SUM(acc, (double)(i0 + start) + off, cnt, MIINT_AT);
  MIINT_BLOCK_SUM(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = MIINT_RED(red);
}

extern "C" __global__ __launch_bounds__(256) void miint_expr_finalize(
    const double* partials, int n, double scale, double* out) {
  MIINT_CLOSE(partials, n, scale, out[0]);
}
)";
}

std::string expr_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_source(expr), expr);
}

ExprIntegrator::ExprIntegrator(const std::string& expr, int device, int grid)
    : expr_(expr), device_(device), grid_(checked_grid(grid)),
      stream_((set_device(device), Stream())),
      module_(expr_compile(expr), device, stream_,
              {"miint_expr_partials", "miint_expr_finalize"}) {
  DeviceGuard g(device);
  partials_ = DeviceBuffer<double>(static_cast<size_t>(grid));
  out_ = DeviceBuffer<double>(1);
  host_ = PinnedBuffer<double>(1);
}

void ExprIntegrator::enqueue(double a, double h, double off, uint64_t begin, uint64_t count,
                             double scale, hipStream_t s) {
  module_.launch(kPartials, grid_, 1, kExprBlock, s, a, h, off, begin, count, partials_.get());
  module_.launch(kFinalize, 1, 1, kExprBlock, s, partials_.get(), grid_, scale, out_.get());
}

// Before anything is launched: the slice lies in [0, n) (begin + count may not wrap), and no
// lane's share of it passes the kernel's 32-bit per-lane count (expr_sweep_shape's condition).
void ExprIntegrator::check(uint64_t n, uint64_t begin, uint64_t count) const {
  detail::check_slice("expression", n, begin, count);
  detail::check_lane_count("expression", count, static_cast<uint64_t>(grid_) * kExprBlock);
}

double ExprIntegrator::integrate(double a, double b, uint64_t n, Rule rule, uint64_t begin,
                                 uint64_t count, double scale, const Comm* comm) {
  check(n, begin, count);
  DeviceGuard g(device_);
  const double h = (b - a) / static_cast<double>(n);
  hipStream_t s = stream_.get();
  enqueue(a, h, rule_offset(rule), begin, count, h * scale, s);
  if (comm && comm->world() > 1) comm->allreduce_sum(out_.get(), out_.get(), 1, s);
  MIINT_HIP(hipMemcpyAsync(host_.get(), out_.get(), sizeof(double), hipMemcpyDeviceToHost, s));
  stream_.sync();
  return host_[0];
}

double ExprIntegrator::time(double a, double b, uint64_t n, Rule rule, uint64_t begin,
                            uint64_t count, int iters, const std::function<void()>& at_start,
                            const std::function<void()>& at_end) {
  MIINT_CHECK(iters >= 1, "bad expression timing request");
  check(n, begin, count);
  DeviceGuard g(device_);
  const double h = (b - a) / static_cast<double>(n);
  hipStream_t s = stream_.get();
  return detail::time_enqueues(
      stream_, e0_, e1_, iters,
      [&] { enqueue(a, h, rule_offset(rule), begin, count, h, s); }, at_start, at_end);
}

}  // namespace miint
