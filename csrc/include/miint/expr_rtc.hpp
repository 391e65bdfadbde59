// What the run-time expression families (miint/expr.hpp: ExprIntegrator, ExprSweep, ExprScan,
// ExprIntegrator2D) and their host counterparts share: the cached hipRTC compile, the owner
// of a loaded module, the timing loop, the argument checks and the device prelude; and what the
// adaptive families (ExprAdaptive, ExprAdaptiveSweep, ExprAdaptiveOsc, ExprAdaptive2D,
// ExprAdaptiveRegion) share on top of that: the rules' text, the printer of an evaluation kernel,
// the one source of a round's other kernels and the host engine of the rounds, AdaptRounds
// (expr_adaptive_rounds.cpp). ExprAdaptiveSweep's rounds are its own. Internal.
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

// The adaptive 2-D families' rule (expr_adaptive2d.cpp): the table, a row's fifteen evaluations
// (with `columns` a pair's macro also takes the numbers of its two columns, as ExprAdaptiveRegion's
// macros want them) and the end of miint_gk15x15's row loop and of the rule. adapt2d_eval_source
// is adapt_eval_source for a rectangle: `rule` is called on (xs[i], ys[i]).
std::string adapt2d_table_source();
std::string adapt2d_row_source(bool columns);
extern const char* const kAdapt2DCombine;
std::string adapt2d_eval_source(const std::string& comment, const std::string& name,
                                const std::string& rule);

// "%a" and "%.17g" of v, and the double whose bits are w.
std::string hex(double v);
std::string num(double v);
double word_as_double(unsigned long long w);
// The refusals every adaptive family words alike, `what` in front: rtol and atol, then
// max_intervals; and max_depth, `per` behind it.
void adapt_check_tolerances(const std::string& what, double rtol, double atol,
                            uint64_t max_intervals);
void adapt_check_depth(const std::string& what, int max_depth, const char* per = "");

// An evaluation kernel of a round (expr_adaptive_rounds.cpp), printed: `comment`, then kernel
// `name` over `params` (n first; k, err, r and part_k among them). Lane i < n runs `call`, whole
// lines that load item i and leave K, err and R in v, e and a (declared by the call but for v),
// and stores them, `stores` (whole lines, such as dir[i]) between err and r; the workgroup's
// MIINT_BLOCK_SUM of v goes to part_k.
std::string adapt_eval_source(const std::string& comment, const std::string& name,
                              const std::string& params, const std::string& call,
                              const std::string& stores = "");
// A round's source behind the rule, for intervals (dims 1, miint_adapt_*) or rectangles (dims 2,
// miint_adapt2d_*): MIINT_ST_D and _init, the family's evaluation kernel `eval`, then _close,
// _decide, _prefix and _scatter, one text with the dimension's own parts passed into it.
std::string adapt_round_source(int dims, const std::string& eval);

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

// One call of the adaptive rounds, checked by the caller. Per axis lo < hi; y0, y1 and py are
// read in two dimensions only, `descending` in one.
struct AdaptJob {
  double x0, x1, y0, y1;
  uint64_t px, py;         // the first list: px (x py) equal panels
  double rtol, atol;
  uint64_t max_intervals;
  int max_depth;           // per axis
  double* out;             // device memory for the partition (2 or 4 doubles an item), or null
  uint64_t capacity;       // items `out` holds
  bool descending;         // the partition from x1 down to x0, every pair swapped
};

// What an evaluation launch works on: n items in `blocks` workgroups of 256 on `stream`.
struct AdaptItems {
  hipStream_t stream;
  unsigned blocks;
  unsigned long long n;
  const double2 *xs, *ys;  // the extents per axis (ys null in one dimension)
  const unsigned* depth;
  double *k, *err, *r;     // per item
  double2* dir;            // per item, two dimensions only
  double* part_k;          // per workgroup
};

// The rounds of ExprAdaptive, ExprAdaptiveOsc (dims 1), ExprAdaptive2D and ExprAdaptiveRegion
// (dims 2): the stream, the lists and buffers, the state and its pinned record, the events and
// the module of adapt_round_source's kernels. A round is the caller's evaluation launch, then
// _close, _decide, _prefix and _scatter, one sync and a look at the record.
// The contract of an evaluation launch: enqueued on AdaptItems::stream, it stores K, err and R
// (and in two dimensions dir = (ex, ey)) of every item, and per workgroup of 256 items the sum
// of its K in MIINT_BLOCK_SUM's order to part_k (adapt_eval_source prints such a kernel).
// The helpers that need the option structs are declared beside them in miint/expr.hpp:
// detail::adapt_job, detail::adapt2d_integrate and detail::adapt2d_time.
class AdaptRounds {
 public:
  enum { kInit, kEval, kClose, kDecide, kPrefix, kScatter };  // module()'s kernels
  using Eval = std::function<void(const AdaptItems&)>;
  // `code` holds the five kernels of adapt_round_source(dims, ...) and the kernel `eval`.
  AdaptRounds(int dims, const std::string& code, const char* eval, int device);
  // Every buffer holds max_intervals items (or their workgroups): sized once for the largest
  // max_intervals asked so far and kept across calls.
  void reserve(uint64_t max_intervals);
  // Throws unless `out` is null or holds max_intervals items. No device needed.
  void check_capacity(const double* out, uint64_t capacity, uint64_t max_intervals) const;
  // The rounds of one call; `evals_per` counts f per item. The partition goes to job.out in
  // acceptance order. Result is AdaptResult or Adapt2DResult (miint/expr.hpp).
  template <class Result>
  Result run(const AdaptJob& job, uint64_t evals_per, const Eval& eval);
  // run() between the two events (device_ms), then the partition ordered on the host: by lower
  // end (or `descending`) in one dimension, by (y0, x0) in two.
  template <class Result>
  Result integrate(const AdaptJob& job, uint64_t evals_per, const Eval& eval);
  // Device ms per `once()`, which enqueues on stream(): time_enqueues with the engine's events.
  template <class Enqueue>
  double time(int iters, Enqueue&& once) {
    return time_enqueues(stream_, e0_, e1_, iters, once);
  }
  int device() const { return device_; }
  const Stream& stream() const { return stream_; }
  const RtcModule& module() const { return module_; }

 private:
  void order(const AdaptJob& job, uint64_t count);
  int dims_, device_;
  std::string what_;  // "adaptive" or "adaptive 2-D", in front of every message
  Stream stream_;
  uint64_t reserved_ = 0;
  DeviceBuffer<double> xs_[2], ys_[2];  // (lo, hi) pairs per axis: 2 x max_intervals doubles each
  DeviceBuffer<unsigned> depth_[2];     // two dimensions: x depth | y depth << 16
  DeviceBuffer<double> k_, err_, r_;    // per item
  DeviceBuffer<double> dir_;            // per rectangle: (ex, ey)
  DeviceBuffer<unsigned char> split_;   // per item: 0 accepted, 1 bisect (x), 2 bisect y
  DeviceBuffer<double> part_k_, blk_sums_;  // per workgroup: 1 and 5 doubles
  DeviceBuffer<unsigned> blk_counts_, blk_off_;  // per workgroup: 4 or 5 counters; the split prefix
  DeviceBuffer<unsigned long long> state_;   // the totals and counters (expr_adaptive_rounds.cpp)
  PinnedBuffer<unsigned long long> record_;  // the same words, stored by the prefix kernel
  Event e0_, e1_;
  RtcModule module_;  // the last member: destroyed first (see RtcModule)
};

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
