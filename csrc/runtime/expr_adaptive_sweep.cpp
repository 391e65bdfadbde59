// Adaptive Gauss-Kronrod (7, 15) integration of f(x, p0..p7) for K parameter rows, each to its
// own tolerance, in shared rounds (see miint/expr.hpp, ExprAdaptiveSweep).
#include <algorithm>
#include <cmath>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kBlock = 256;
constexpr unsigned kWavesPerBlock = 4;
enum { kInit, kEval, kRow, kPrefix, kScatter };  // module_'s kernels

// A row's sixteen words: 0..4 are doubles, the rest counters.
enum { kS, kE, kR, kTol, kSumK, kEvals, kRounds };
enum { kAccepted = 8, kSplits, kFloor, kForced, kNonfinite, kNext, kCapped };
constexpr size_t kRowWords = 16;
enum { kRecTotal, kRecActive, kRecordWords };

using detail::num;
using detail::word_as_double;

int checked_nparams(int nparams) {
  MIINT_CHECK(nparams >= 0 && nparams <= kSweepMaxParams,
              "adaptive sweep: nparams = " + std::to_string(nparams) + " must be 0.." +
                  std::to_string(kSweepMaxParams));
  return nparams;
}

// The parameters' three spellings: ", double p0, ..." in a signature, "const double p0 = pr[0];
// ..." as a kernel's loads of its row, ", p0, ..." at a call.
struct ParamText {
  std::string sig, load, args;
  explicit ParamText(int nparams) {
    for (int j = 0; j < checked_nparams(nparams); ++j) {
      const std::string p = "p" + std::to_string(j);
      sig += ", double " + p;
      load += "  const double " + p + " = pr[" + std::to_string(j) + "];\n";
      args += ", " + p;
    }
  }
};
}  // namespace

uint64_t adapt_sweep_default_panels(uint64_t rows) {
  uint64_t p = kAdaptDefaultPanels;
  while (p > kAdaptSweepMinPanels && rows * p > kAdaptSweepInitialTotal) p >>= 1;
  return p;
}

AdaptSweepOptions adapt_sweep_check(uint64_t rows, int nparams, uint64_t param_count, double a,
                                    double b, const AdaptSweepOptions& opt) {
  const std::string what = "adaptive sweep: ";
  MIINT_CHECK(rows <= kSweepMaxRows, what + "rows = " + std::to_string(rows) + " must be 0..2^20");
  checked_nparams(nparams);
  MIINT_CHECK(param_count == rows * static_cast<uint64_t>(nparams),
              what + std::to_string(param_count) + " parameter values for " +
                  std::to_string(rows) + " rows of " + std::to_string(nparams));
  MIINT_CHECK(opt.max_total >= 1 && opt.max_total <= kAdaptSweepMaxTotalLimit,
              what + "max_total = " + std::to_string(opt.max_total) + " must be 1..2^26");
  AdaptSweepOptions o = opt;
  const uint64_t k = std::max<uint64_t>(rows, 1);
  if (o.max_intervals == 0) o.max_intervals = o.max_total / k;
  if (o.panels == 0) o.panels = adapt_sweep_default_panels(k);
  MIINT_CHECK(o.panels >= 1 && o.panels <= o.max_intervals,
              what + "panels = " + std::to_string(o.panels) + " must be 1..max_intervals = " +
                  std::to_string(o.max_intervals) + " (per row)");
  MIINT_CHECK(o.max_intervals <= o.max_total / k,
              what + "rows * max_intervals = " + std::to_string(rows) + " * " +
                  std::to_string(o.max_intervals) + " passes max_total = " +
                  std::to_string(o.max_total));
  AdaptOptions one;
  one.rtol = o.rtol;
  one.atol = o.atol;
  one.panels = o.panels;
  one.max_depth = o.max_depth;
  one.max_intervals = o.max_intervals;
  one.unbounded = o.unbounded;
  adapt_check(a, b, one);
  return o;
}

std::string expr_adapt_sweep_source(const std::string& expr, int nparams) {
  detail::expr_check_named(expr);
  const ParamText params(nparams);
  return std::string(detail::kRtcPrelude) +
         detail::adapt_rule_source(expr, params.sig, params.args) +
         "\n#define MIINT_NPARAMS " + std::to_string(nparams) + "u\n" + R"(
// A row's words: 0..4 as doubles S_acc, E_acc, R_acc, tol, sum_K; 5 evals, 6 the last round the
// row was active in; 8..14: accepted, splits, floor, forced, nonfinite, next, capped.
#define MIINT_ROW_WORDS 16ull
#define MIINT_NO_RANK 0xffffffffu
// The 64-lane butterfly of MIINT_BLOCK_SUM on its own: every lane ends with the wave's sum.
#define MIINT_WAVE_SUM(v) for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64)

// The first list: interval j of row r at r * panels + j, edges a + ((b - a) j) / panels, the
// last one b (ExprAdaptive's formula); the first `rows` lanes also write the rows' segments and
// the list of active rows.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_init(
    double a, double b, unsigned rows, unsigned panels, double2* __restrict__ list,
    unsigned* __restrict__ depth, unsigned* __restrict__ row, unsigned* __restrict__ active,
    unsigned* __restrict__ seg_start, unsigned* __restrict__ seg_len) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= (unsigned long long)rows * panels) return;
  const unsigned r = (unsigned)(i / panels), j = (unsigned)(i % panels);
  const double w = b - a, p = (double)panels;
  const double lo = a + (w * (double)j) / p;
  const double hi = j + 1u == panels ? b : a + (w * (double)(j + 1u)) / p;
  list[i] = make_double2(lo, hi);
  depth[i] = 0u;
  row[i] = r;
  if (i < rows) {
    active[i] = (unsigned)i;
    seg_start[i] = (unsigned)i * panels;
    seg_len[i] = panels;
  }
}

// One interval per lane: its row's parameters (per-lane loads, never written here), then the
// same fifteen evaluations in every lane.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_eval(
    unsigned n, const double2* __restrict__ list, const unsigned* __restrict__ row,
    const double* __restrict__ params, double* __restrict__ k, double* __restrict__ err,
    double* __restrict__ r) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const double2 iv = list[i];
  const double* __restrict__ pr = params + (unsigned long long)row[i] * MIINT_NPARAMS;
  (void)pr;
)" + params.load + R"(  double v, e, s;
  miint_gk15(iv.x, iv.y)" + params.args + R"(, &v, &e, &s);
  k[i] = v;
  err[i] = e;
  r[i] = s;
}

// One wave per active row (miint/expr.hpp has the order of every sum). `round` counts from 1.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_row(
    unsigned na, const unsigned* __restrict__ active, const unsigned* __restrict__ seg_start,
    const unsigned* __restrict__ seg_len, const double2* __restrict__ list,
    const double* __restrict__ k, const double* __restrict__ err, const double* __restrict__ r,
    const unsigned* __restrict__ depth, double width, double rtol, double atol,
    unsigned max_depth, unsigned long long max_intervals, unsigned long long round,
    unsigned long long* __restrict__ st, unsigned* __restrict__ rank,
    unsigned* __restrict__ next_len) {
  const unsigned slot = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (slot >= na) return;  // the whole wave
  const unsigned lane = threadIdx.x & 63u;
  const unsigned row = active[slot];
  const unsigned s0 = seg_start[row], len = seg_len[row];
  unsigned long long* rs = st + MIINT_ROW_WORDS * row;
  double sum_k = 0.0;
  for (unsigned e = lane; e < len; e += 64u) sum_k += k[s0 + e];
  MIINT_WAVE_SUM(sum_k);
  const double t = rtol * fabs(((const double*)rs)[0] + sum_k);
  const double tol = atol > t ? atol : t;  // a NaN sum: a NaN tolerance
  double ak = 0.0, ae = 0.0, ar = 0.0, pk = 0.0, pe = 0.0;
  unsigned n_split = 0, n_floor = 0, n_forced = 0, n_nonfinite = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (unsigned base = 0; base < len; base += 64u) {  // uniform: every lane takes every ballot
    const unsigned e = base + lane;
    int how = 0;  // 1 nonfinite, 2 within tolerance, 3 floor, 4 forced, 5 split
    if (e < len) {
      const unsigned i = s0 + e;
      const double2 iv = list[i];
      const double kv = k[i], ev = err[i], rv = r[i];
      const double w = iv.y - iv.x, c = iv.x + 0.5 * w;
      if (!(isfinite(kv) && isfinite(ev))) how = 1;
      else if (!(ev > (tol * w) / width)) how = 2;
      else if (ev <= 0x1.9p-47 * rv) how = 3;  // 50 * 2^-52
      else if (depth[i] >= max_depth || c == iv.x || c == iv.y) how = 4;
      else how = 5;
      if (how == 5) {
        pk += kv;
        pe += ev;
      } else {
        ak += kv;
        ae += ev;
        ar += rv;
      }
    }
    const unsigned long long m_split = __ballot(how == 5);
    if (e < len)
      rank[s0 + e] = how == 5 ? n_split + (unsigned)__popcll(m_split & below) : MIINT_NO_RANK;
    n_split += (unsigned)__popcll(m_split);
    n_floor += (unsigned)__popcll(__ballot(how == 3));
    n_forced += (unsigned)__popcll(__ballot(how == 4));
    n_nonfinite += (unsigned)__popcll(__ballot(how == 1));
  }
  MIINT_WAVE_SUM(ak);
  MIINT_WAVE_SUM(ae);
  MIINT_WAVE_SUM(ar);
  MIINT_WAVE_SUM(pk);
  MIINT_WAVE_SUM(pe);
  if (lane != 0u) return;
  const unsigned long long accepted = rs[8], n = len, ns = n_split;
  const bool capped = accepted + (n - ns) + 2ull * ns > max_intervals;
  double* rd = (double*)rs;
  if (capped) {  // nothing is split: the pending K and err join the round's sums
    ak += pk;
    ae += pe;
  }
  rd[0] += ak;
  rd[1] += ae;
  rd[2] += ar;
  rd[3] = tol;
  rd[4] = sum_k;
  rs[5] += 15ull * n;
  rs[6] = round;
  rs[8] = accepted + (capped ? n : n - ns);
  rs[9] += capped ? 0ull : ns;
  rs[10] += n_floor;
  rs[11] += n_forced;
  rs[12] += n_nonfinite;
  rs[13] = capped ? 0ull : 2ull * ns;
  rs[14] = capped ? 1ull : 0ull;
  next_len[slot] = capped ? 0u : 2u * n_split;
}

// One workgroup over the na active rows. Thread t owns the contiguous run of per =
// ceil(na / 256) slots from t * per: the sum of their next lengths and the number that stay
// active; thread 0 scans the 256 runs and stores the record; every thread then walks its run
// again and writes, for each row that stays active, its next segment and its place in the
// next list of active rows. Integers only: exact in any order.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_prefix(
    unsigned na, const unsigned* __restrict__ active, const unsigned* __restrict__ next_len,
    unsigned* __restrict__ seg_start, unsigned* __restrict__ seg_len,
    unsigned* __restrict__ next_active, unsigned long long* __restrict__ record) {
  __shared__ unsigned run_len[256];
  __shared__ unsigned run_cnt[256];
  const unsigned per = (na + 255u) / 256u;
  const unsigned first = threadIdx.x * per < na ? threadIdx.x * per : na;
  const unsigned last = first + per < na ? first + per : na;
  unsigned l = 0, c = 0;
  for (unsigned j = first; j < last; ++j) {
    const unsigned nl = next_len[j];
    l += nl;
    c += nl != 0u ? 1u : 0u;
  }
  run_len[threadIdx.x] = l;
  run_cnt[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tl = 0, tc = 0;
    for (int t = 0; t < 256; ++t) {
      const unsigned vl = run_len[t], vc = run_cnt[t];
      run_len[t] = tl;
      run_cnt[t] = tc;
      tl += vl;
      tc += vc;
    }
    record[0] = tl;
    record[1] = tc;
  }
  __syncthreads();
  unsigned off = run_len[threadIdx.x], q = run_cnt[threadIdx.x];
  for (unsigned j = first; j < last; ++j) {
    const unsigned nl = next_len[j];
    if (nl == 0u) continue;
    const unsigned row = active[j];
    seg_start[row] = off;
    seg_len[row] = nl;
    next_active[q] = row;
    off += nl;
    ++q;
  }
}

// Children (lo, c), (c, hi) at depth + 1 to slots start + 2 rank, + 1 of the next list, start
// the row's next segment start (miint_asweep_prefix). A row whose round was capped splits
// nothing. Nothing is stored at or past next_cap.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_scatter(
    unsigned n, const double2* __restrict__ list, const unsigned* __restrict__ depth,
    const unsigned* __restrict__ row, const unsigned* __restrict__ rank,
    const unsigned* __restrict__ seg_start, const unsigned long long* __restrict__ st,
    double2* __restrict__ next, unsigned* __restrict__ next_depth,
    unsigned* __restrict__ next_row, unsigned long long next_cap) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned rk = rank[i];
  if (rk == MIINT_NO_RANK) return;
  const unsigned rw = row[i];
  if (st[MIINT_ROW_WORDS * rw + 14ull] != 0ull) return;
  const unsigned long long q = (unsigned long long)seg_start[rw] + 2ull * rk;
  if (q + 1ull >= next_cap) return;
  const double2 iv = list[i];
  const double c = iv.x + 0.5 * (iv.y - iv.x);
  const unsigned d = depth[i] + 1u;
  next[q] = make_double2(iv.x, c);
  next[q + 1ull] = make_double2(c, iv.y);
  next_depth[q] = d;
  next_depth[q + 1ull] = d;
  next_row[q] = rw;
  next_row[q + 1ull] = rw;
}
)";
}

std::string expr_adapt_sweep_unbounded_source(const std::string& expr, int nparams) {
  detail::expr_check_named(expr);
  const ParamText params(nparams);
  std::string src = std::string(detail::kRtcPrelude) +
                    detail::adapt_unbounded_rule_source(expr, params.sig, params.args) +
                    "\n#define MIINT_NPARAMS " + std::to_string(nparams) + "u\n";
  // miint_asweep_eval's twins: the interval is one of t in [0, 1] (miint/expr.hpp has the map).
  const char* names[3] = {"upper", "lower", "both"};
  for (int kind = 1; kind <= 3; ++kind)
    src += std::string(R"(
extern "C" __global__ __launch_bounds__(256) void miint_asweep_eval_)") + names[kind - 1] + R"((
    unsigned n, const double2* __restrict__ list, const unsigned* __restrict__ row,
    const double* __restrict__ params, double end, double* __restrict__ k,
    double* __restrict__ err, double* __restrict__ r) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const double2 iv = list[i];
  const double* __restrict__ pr = params + (unsigned long long)row[i] * MIINT_NPARAMS;
  (void)pr;
)" + params.load + R"(  double v, e, s;
  miint_gk15(iv.x, iv.y, )" + std::to_string(kind) + ", end" + params.args + R"(, &v, &e, &s);
  k[i] = v;
  err[i] = e;
  r[i] = s;
}
)";
  return src;
}

std::string expr_adapt_sweep_unbounded_compile(const std::string& expr, int nparams) {
  return detail::rtc_compile_cached(expr_adapt_sweep_unbounded_source(expr, nparams), expr);
}

std::string expr_adapt_sweep_compile(const std::string& expr, int nparams) {
  return detail::rtc_compile_cached(expr_adapt_sweep_source(expr, nparams), expr);
}

ExprAdaptiveSweep::ExprAdaptiveSweep(const std::string& expr, int nparams, int device)
    : expr_(expr), nparams_(checked_nparams(nparams)), device_(device),
      stream_((set_device(device), Stream())),
      module_(expr_adapt_sweep_compile(expr, nparams), device, stream_,
              {"miint_asweep_init", "miint_asweep_eval", "miint_asweep_row",
               "miint_asweep_prefix", "miint_asweep_scatter"}) {
  DeviceGuard g(device);
  record_ = PinnedBuffer<unsigned long long>(kRecordWords);
}

// The eval kernels of the infinite kinds: compiled (cached per expression and nparams) and
// loaded once, at the object's first unbounded call.
void ExprAdaptiveSweep::load_unbounded() {
  if (unbounded_) return;
  unbounded_.reset(new detail::RtcModule(
      expr_adapt_sweep_unbounded_compile(expr_, nparams_), device_, stream_,
      {"miint_asweep_eval_upper", "miint_asweep_eval_lower", "miint_asweep_eval_both"}));
}

// The per-interval buffers hold max_total intervals, the per-row ones `rows` rows: sized for
// the largest asked so far and kept across calls.
void ExprAdaptiveSweep::reserve(uint64_t m, uint64_t rows) {
  if (m > reserved_) {
    stream_.sync();
    for (int q = 0; q < 2; ++q) {
      list_[q] = DeviceBuffer<double>(2 * m);
      depth_[q] = DeviceBuffer<unsigned>(m);
      row_[q] = DeviceBuffer<unsigned>(m);
    }
    k_ = DeviceBuffer<double>(m);
    err_ = DeviceBuffer<double>(m);
    r_ = DeviceBuffer<double>(m);
    rank_ = DeviceBuffer<unsigned>(m);
    reserved_ = m;
  }
  if (rows > reserved_rows_) {
    stream_.sync();
    for (int q = 0; q < 2; ++q) active_[q] = DeviceBuffer<unsigned>(rows);
    seg_start_ = DeviceBuffer<unsigned>(rows);
    seg_len_ = DeviceBuffer<unsigned>(rows);
    next_len_ = DeviceBuffer<unsigned>(rows);
    state_ = DeviceBuffer<unsigned long long>(rows * kRowWords);
    params_ = DeviceBuffer<double>(std::max<uint64_t>(rows * nparams_, 1));
    reserved_rows_ = rows;
  }
}

void ExprAdaptiveSweep::upload(const std::vector<double>& params) {
  if (params.empty()) return;
  MIINT_HIP(hipMemcpyAsync(params_.get(), params.data(), params.size() * sizeof(double),
                           hipMemcpyHostToDevice, stream_.get()));
  stream_.sync();  // params is the caller's pageable memory
}

// lo < hi, opt resolved by adapt_sweep_check.
ExprAdaptiveSweep::Call ExprAdaptiveSweep::rounds(double lo, double hi, uint64_t rows,
                                                  const AdaptSweepOptions& opt, AdaptRange kind,
                                                  double end) {
  hipStream_t s = stream_.get();
  const unsigned long long max_iv = opt.max_intervals, cap = reserved_;
  const unsigned max_depth = static_cast<unsigned>(opt.max_depth);
  const double width = hi - lo;
  unsigned long long* st = state_.get();
  unsigned long long* rec = record_.device_ptr();
  MIINT_HIP(hipMemsetAsync(st, 0, rows * kRowWords * sizeof(unsigned long long), s));
  const unsigned k = static_cast<unsigned>(rows), panels = static_cast<unsigned>(opt.panels);
  uint64_t n = rows * opt.panels, na = rows;
  int cur = 0;
  module_.launch(kInit, static_cast<unsigned>((n + kBlock - 1) / kBlock), 1, kBlock, s, lo, hi, k,
                 panels, reinterpret_cast<double2*>(list_[0].get()), depth_[0].get(),
                 row_[0].get(), active_[0].get(), seg_start_.get(), seg_len_.get());
  Call c;
  for (;;) {
    MIINT_CHECK(n >= 1 && n <= opt.max_total && n <= reserved_ && na >= 1 && na <= rows,
                "adaptive sweep: the active list left its bound");
    MIINT_CHECK(c.rounds <= static_cast<uint64_t>(opt.max_depth),
                "adaptive sweep: more rounds than depths");
    const unsigned blocks = static_cast<unsigned>((n + kBlock - 1) / kBlock);
    const unsigned n32 = static_cast<unsigned>(n), na32 = static_cast<unsigned>(na);
    const unsigned long long round = c.rounds + 1;
    const double2* list = reinterpret_cast<const double2*>(list_[cur].get());
    double2* next = reinterpret_cast<double2*>(list_[cur ^ 1].get());
    const unsigned* depth = depth_[cur].get();
    const unsigned* row = row_[cur].get();
    const unsigned* active = active_[cur].get();
    if (kind == AdaptRange::kFinite)
      module_.launch(kEval, blocks, 1, kBlock, s, n32, list, row,
                     static_cast<const double*>(params_.get()), k_.get(), err_.get(), r_.get());
    else  // the twin of the kind: kernels 0, 1, 2 of unbounded_
      unbounded_->launch(static_cast<size_t>(kind) - 1, blocks, 1, kBlock, s, n32, list, row,
                         static_cast<const double*>(params_.get()), end, k_.get(), err_.get(),
                         r_.get());
    module_.launch(kRow, (na32 + kWavesPerBlock - 1) / kWavesPerBlock, 1, kBlock, s, na32, active,
                   static_cast<const unsigned*>(seg_start_.get()),
                   static_cast<const unsigned*>(seg_len_.get()), list,
                   static_cast<const double*>(k_.get()), static_cast<const double*>(err_.get()),
                   static_cast<const double*>(r_.get()), depth, width, opt.rtol, opt.atol,
                   max_depth, max_iv, round, st, rank_.get(), next_len_.get());
    module_.launch(kPrefix, 1, 1, kBlock, s, na32, active,
                   static_cast<const unsigned*>(next_len_.get()), seg_start_.get(),
                   seg_len_.get(), active_[cur ^ 1].get(), rec);
    module_.launch(kScatter, blocks, 1, kBlock, s, n32, list, depth, row,
                   static_cast<const unsigned*>(rank_.get()),
                   static_cast<const unsigned*>(seg_start_.get()),
                   static_cast<const unsigned long long*>(st), next, depth_[cur ^ 1].get(),
                   row_[cur ^ 1].get(), cap);
    stream_.sync();
    ++c.rounds;
    c.evals += 15 * n;
    c.peak = std::max(c.peak, n);
    n = record_[kRecTotal];
    na = record_[kRecActive];
    if (n == 0) break;
    cur ^= 1;
  }
  return c;
}

AdaptSweepResult ExprAdaptiveSweep::integrate(const std::vector<double>& params, uint64_t rows,
                                              double a, double b, const AdaptSweepOptions& opt) {
  const AdaptSweepOptions o = adapt_sweep_check(rows, nparams_, params.size(), a, b, opt);
  AdaptSweepResult r;
  auto size = [&](uint64_t k) {
    for (auto* v : {&r.value, &r.err_est, &r.resabs, &r.tol}) v->assign(k, 0.0);
    for (auto* v : {&r.converged, &r.capped}) v->assign(k, 0);
    for (auto* v : {&r.evals, &r.rounds, &r.intervals, &r.splits, &r.floor, &r.forced,
                    &r.nonfinite})
      v->assign(k, 0);
  };
  size(rows);
  if (rows == 0) return r;
  if (a == b) {
    r.tol.assign(rows, o.atol);
    r.converged.assign(rows, 1);
    return r;
  }
  DeviceGuard g(device_);
  reserve(o.max_total, rows);
  upload(params);
  const bool swapped = a > b;
  const AdaptRange kind = adapt_range(a, b);
  const bool mapped = kind != AdaptRange::kFinite;
  if (mapped) load_unbounded();
  const double end = std::isinf(a) ? b : a;  // the finite end of a half-infinite range
  r.range = adapt_range_name(kind);
  e0_.record(stream_.get());
  const Call c = mapped ? rounds(0.0, 1.0, rows, o, kind, end)
                        : rounds(swapped ? b : a, swapped ? a : b, rows, o);
  e1_.record(stream_.get());
  stream_.sync();
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  r.call_rounds = c.rounds;
  r.call_evals = c.evals;
  r.peak = c.peak;
  std::vector<unsigned long long> st(rows * kRowWords);
  MIINT_HIP(hipMemcpy(st.data(), state_.get(), st.size() * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
  for (uint64_t k = 0; k < rows; ++k) {
    const unsigned long long* w = st.data() + k * kRowWords;
    const double v = word_as_double(w[kS]);
    r.value[k] = swapped ? -v : v;
    r.err_est[k] = word_as_double(w[kE]);
    r.resabs[k] = word_as_double(w[kR]);
    r.tol[k] = word_as_double(w[kTol]);
    r.evals[k] = w[kEvals];
    r.rounds[k] = w[kRounds];
    r.intervals[k] = w[kAccepted];
    r.splits[k] = w[kSplits];
    r.floor[k] = w[kFloor];
    r.forced[k] = w[kForced];
    r.nonfinite[k] = w[kNonfinite];
    r.capped[k] = w[kCapped] != 0;
    r.converged[k] = r.err_est[k] <= r.tol[k] && !r.capped[k] && r.nonfinite[k] == 0;
  }
  return r;
}

double ExprAdaptiveSweep::time(const std::vector<double>& params, uint64_t rows, double a,
                               double b, const AdaptSweepOptions& opt, int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive sweep timing request");
  const AdaptSweepOptions o = adapt_sweep_check(rows, nparams_, params.size(), a, b, opt);
  if (rows == 0 || a == b) return 0.0;
  DeviceGuard g(device_);
  reserve(o.max_total, rows);
  upload(params);
  const AdaptRange kind = adapt_range(a, b);
  if (kind != AdaptRange::kFinite) {
    load_unbounded();
    const double end = std::isinf(a) ? b : a;
    return detail::time_enqueues(stream_, e0_, e1_, iters,
                                 [&] { (void)rounds(0.0, 1.0, rows, o, kind, end); });
  }
  const double lo = std::min(a, b), hi = std::max(a, b);
  return detail::time_enqueues(stream_, e0_, e1_, iters, [&] { (void)rounds(lo, hi, rows, o); });
}

}  // namespace miint
