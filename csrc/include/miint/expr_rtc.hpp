// What the run-time expression families (miint/expr.hpp: ExprIntegrator, ExprSweep, ExprScan,
// ExprIntegrator2D) and their host counterparts share: the cached hipRTC compile, the owner
// of a loaded module, the timing loop, the argument checks and the device prelude. Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "miint/runtime.hpp"

namespace miint {
namespace detail {

// detail::rtc_compile (miint/expr.hpp) of `src`, once per source text in the process.
std::string rtc_compile_cached(const std::string& src, const std::string& expr);

// Device text in front of every family's generated source: the block reduction, the closing
// step, the lane split and the per-sample loop, each described where it is written.
extern const char* const kRtcPrelude;

// The adaptive families' shared device text (expr_adaptive.cpp): miint_f(x<sig>) for `expr`, the
// MIINT_GK_* macros and miint_gk15(lo, hi<sig>, &k, &err, &r) on the rule's one table. `sig` is
// "" or ", double p0, ..." and `args` the matching "" or ", p0, ...": ExprAdaptive and
// ExprAdaptiveSweep evaluate the same fifteen nodes in the same order.
std::string adapt_rule_source(const std::string& expr, const std::string& sig,
                              const std::string& args);
// The same text for an infinite range (miint/expr.hpp, AdaptRange): `expr` becomes
// miint_user_f(x<sig>), miint_f the map's g(t) around it, and miint_gk15 takes the kind (1 upper,
// 2 lower, 3 both) and the finite end after hi: miint_gk15(lo, hi, kind, end<args>, &k, &err, &r).
std::string adapt_unbounded_rule_source(const std::string& expr, const std::string& sig,
                                        const std::string& args);

// The adaptive 2-D families' shared device text (expr_adaptive2d.cpp): ExprAdaptive2D's source is
// the prelude, miint_f, the table, the row macros and miint_gk15x15 (its row loop printed by
// adapt2d_row_source, closed by kAdapt2DCombine), kAdapt2DInit, the evaluation kernel and
// kAdapt2DRound. ExprAdaptiveRegion replaces the function, the macros, the rule and the
// evaluation kernel and carries the rest as it stands. adapt2d_row_source(true) also passes a
// pair's two column numbers to its macro.
std::string adapt2d_table_source();
std::string adapt2d_row_source(bool columns);
extern const char* const kAdapt2DCombine;
extern const char* const kAdapt2DInit;
extern const char* const kAdapt2DRound;

// A loaded code object and its kernels. The destructor selects the device, drains the owning
// object's stream and unloads: declare it as the owner's LAST member, after the Stream, the
// buffers and the events, so that member order destroys it first (nothing a kernel may still
// use is freed before the drain, and the stream it drains is still alive).
class RtcModule {
 public:
  RtcModule(const std::string& code, int device, const Stream& stream,
            std::initializer_list<const char*> kernels);
  ~RtcModule();
  RtcModule(const RtcModule&) = delete;
  RtcModule& operator=(const RtcModule&) = delete;
  // Enqueue kernel i (in the order of `kernels`) on `s`: gx x gy workgroups of `block` threads.
  // The arguments are passed by address: each must have exactly its kernel parameter's type.
  template <class... Args>
  void launch(size_t i, unsigned gx, unsigned gy, unsigned block, hipStream_t s,
              Args... args) const {
    void* ptrs[] = {&args...};
    MIINT_HIP(hipModuleLaunchKernel(fns_[i], gx, gy, 1, block, 1, 1, 0, s, ptrs, nullptr));
  }

 private:
  int device_;
  const Stream& stream_;
  hipModule_t module_ = nullptr;
  std::vector<hipFunction_t> fns_;
};

// Device ms per `once()` over `iters` back-to-back ones (events, no host sync between them),
// after one warm-up. at_start runs on the host right before the first event is recorded,
// at_end right before the last one.
template <class Enqueue>
double time_enqueues(const Stream& stream, Event& e0, Event& e1, int iters, Enqueue&& once,
                     const std::function<void()>& at_start = {},
                     const std::function<void()>& at_end = {}) {
  once();  // warm
  stream.sync();
  if (at_start) at_start();
  e0.record(stream.get());
  for (int i = 0; i < iters; ++i) once();
  if (at_end) at_end();
  e1.record(stream.get());
  stream.sync();
  return Event::elapsed_ms(e0, e1) / iters;
}

// n >= 1 and [begin, begin + count) lies in [0, n) without wrapping.
inline bool slice_in_range(uint64_t n, uint64_t begin, uint64_t count) {
  return n >= 1 && begin + count >= begin && begin + count <= n;
}
// The checks throw with `what`, the caller's name for itself, in front of the message:
// "<what> slice outside [0, n)" unless slice_in_range; a lane's share of `samples` over
// `lanes` lanes past the kernels' 32-bit per-lane count; nx outside [1, 2^32); and, after nx,
// ny outside [1, 2^40] or rows [row_begin, row_begin + row_count) not in [0, ny) (wrapping).
void check_slice(const std::string& what, uint64_t n, uint64_t begin, uint64_t count);
void check_lane_count(const std::string& what, uint64_t samples, uint64_t lanes);
void check_2d_nx(const std::string& what, uint64_t nx);
void check_2d_range(const std::string& what, uint64_t nx, uint64_t ny, uint64_t row_begin,
                    uint64_t row_count);

}  // namespace detail
}  // namespace miint
