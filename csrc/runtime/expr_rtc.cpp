// The layer under the run-time expression families (see miint/expr_rtc.hpp).
#include "miint/expr_rtc.hpp"

#include <hip/hiprtc.h>

#include <map>
#include <mutex>

#include "miint/expr.hpp"

namespace miint {
namespace detail {

std::string rtc_compile(const std::string& src, const std::string& expr) {
  auto rtc_error = [](hiprtcResult r) { return std::string(hiprtcGetErrorString(r)); };
  hiprtcProgram prog = nullptr;
  hiprtcResult r = hiprtcCreateProgram(&prog, src.c_str(), "miint_expr.hip", 0, nullptr, nullptr);
  MIINT_CHECK(r == HIPRTC_SUCCESS, "hiprtcCreateProgram: " + rtc_error(r));
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
  r = hiprtcCompileProgram(prog, 3, opts);
  size_t log_n = 0;
  hiprtcGetProgramLogSize(prog, &log_n);
  std::string log(log_n, '\0');
  if (log_n) hiprtcGetProgramLog(prog, &log[0]);
  if (r != HIPRTC_SUCCESS) {
    hiprtcDestroyProgram(&prog);
    fail("expression '" + expr + "' does not compile: " + log, __FILE__, __LINE__);
  }
  size_t code_n = 0;
  MIINT_CHECK(hiprtcGetCodeSize(prog, &code_n) == HIPRTC_SUCCESS && code_n > 0,
              "hiprtcGetCodeSize");
  std::string code(code_n, '\0');
  MIINT_CHECK(hiprtcGetCode(prog, &code[0]) == HIPRTC_SUCCESS, "hiprtcGetCode");
  hiprtcDestroyProgram(&prog);
  return code;
}

// Keyed on the whole source text: the family, the expression and the parameter count are all
// in it, so two families (or two parameter counts) can never share an entry.
std::string rtc_compile_cached(const std::string& src, const std::string& expr) {
  static std::mutex mu;
  static std::map<std::string, std::string> cache;  // source -> code object
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(src);
  if (it != cache.end()) return it->second;
  return cache[src] = rtc_compile(src, expr);
}

// hipRTC compiles this with its own HIP headers (device math, __shfl_xor, blockIdx, ...).
const char* const kRtcPrelude = R"(
// The block reduction of v (256 threads): wave64 butterfly, then the four waves' sums through
// red, four doubles of LDS, one barrier; thread 0 then reads the sum as MIINT_RED(red). Text:
// as an inlined function it moved a shift in every kernel and changed the instructions of
// the two that alternate between two rows of red in a loop.
#define MIINT_BLOCK_SUM(v, red)                               \
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); \
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;     \
  __syncthreads()
#define MIINT_RED(red) ((red[0] + red[1]) + (red[2] + red[3]))

// The closing kernels' body. One workgroup: thread t sums p[t], p[t + 256], ... in order;
// fixed-order tree after; thread 0 stores sum * scale.
#define MIINT_CLOSE(p, n, scale, dst)                     \
  __shared__ double red[4];                               \
  double v = 0.0;                                         \
  for (int i = threadIdx.x; i < n; i += 256) v += p[i];   \
  MIINT_BLOCK_SUM(v, red);                                \
  if (threadIdx.x == 0) dst = MIINT_RED(red) * scale

// Lane g of gridDim.x * 256 owns a contiguous run of the n samples (balanced: the first
// n mod lanes lanes take one more): *start, and the count as the value.
__device__ __forceinline__ unsigned miint_lane_share(unsigned long long n,
                                                     unsigned long long* start) {
  const unsigned long long lanes = (unsigned long long)gridDim.x * 256ull;
  const unsigned long long g = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long q = n / lanes, r = n % lanes;
  *start = g * q + (g < r ? g : r);
  return (unsigned)(q + (g < r ? 1ull : 0ull));
}

// double acc = the sum of f(idx) over cnt samples from index idx0, every sample on its own.
// The run is walked with an exact fp64 index (idx += 1, exact below 2^52), so a sample costs
// f's fma(idx, h, a), f and an add: no per-sample 64-bit integer to fp64 conversion. Four
// independent accumulators for ILP. f is a macro of the index. Text: as a template called
// with a lambda the operands of two adds in one sweep's loop came out swapped.
#define MIINT_SAMPLE_SUM(acc, idx0, cnt, f)        \
  double acc;                                      \
  {                                                \
    double idx = idx0;                             \
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0; \
    unsigned c = 0;                                \
    for (; c + 4 <= cnt; c += 4) {                 \
      a0 += f(idx);                                \
      a1 += f(idx + 1.0);                          \
      a2 += f(idx + 2.0);                          \
      a3 += f(idx + 3.0);                          \
      idx += 4.0;                                  \
    }                                              \
    for (; c < cnt; ++c) {                         \
      a0 += f(idx);                                \
      idx += 1.0;                                  \
    }                                              \
    acc = (a0 + a1) + (a2 + a3);                   \
  }
)";

RtcModule::RtcModule(const std::string& code, int device, const Stream& stream,
                     std::initializer_list<const char*> kernels)
    : device_(device), stream_(stream) {
  DeviceGuard g(device);
  MIINT_HIP(hipModuleLoadData(&module_, code.data()));
  for (const char* name : kernels) {
    fns_.push_back(nullptr);
    MIINT_HIP(hipModuleGetFunction(&fns_.back(), module_, name));
  }
}

RtcModule::~RtcModule() {
  if (module_) {
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_.get());
    (void)hipModuleUnload(module_);
  }
}

void check_slice(const std::string& what, uint64_t n, uint64_t begin, uint64_t count) {
  MIINT_CHECK(slice_in_range(n, begin, count), what + " slice outside [0, n)");
}

void check_lane_count(const std::string& what, uint64_t samples, uint64_t lanes) {
  MIINT_CHECK(samples / lanes + 1 < (1ull << 32),
              what + ": " + std::to_string(samples) + " samples over " + std::to_string(lanes) +
                  " lanes pass the 32-bit per-lane count; use a larger grid or slice the "
                  "samples");
}

void check_2d_nx(const std::string& what, uint64_t nx) {
  MIINT_CHECK(nx >= 1 && nx <= kExpr2DMaxNx,
              what + ": nx = " + std::to_string(nx) + " must be 1..2^32 - 1");
}

void check_2d_range(const std::string& what, uint64_t nx, uint64_t ny, uint64_t row_begin,
                    uint64_t row_count) {
  check_2d_nx(what, nx);
  MIINT_CHECK(ny >= 1 && ny <= kExpr2DMaxNy,
              what + ": ny = " + std::to_string(ny) + " must be 1..2^40");
  MIINT_CHECK(row_begin + row_count >= row_begin && row_begin + row_count <= ny,
              what + ": rows [" + std::to_string(row_begin) + ", " + std::to_string(row_begin) +
                  " + " + std::to_string(row_count) + ") outside [0, " + std::to_string(ny) +
                  ")");
}

}  // namespace detail
}  // namespace miint
