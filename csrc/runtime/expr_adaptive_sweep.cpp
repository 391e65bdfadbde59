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
enum { kInitRanges, kRowRanges, kCurvePrefix };   // ranged_'s

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

// A result of k rows, every field zero.
AdaptSweepResult zero_rows(uint64_t k) {
  AdaptSweepResult r;
  for (auto* v : {&r.value, &r.err_est, &r.resabs, &r.tol}) v->assign(k, 0.0);
  for (auto* v : {&r.converged, &r.capped}) v->assign(k, 0);
  for (auto* v : {&r.evals, &r.rounds, &r.intervals, &r.splits, &r.floor, &r.forced,
                  &r.nonfinite})
    v->assign(k, 0);
  return r;
}

// The body of miint_asweep_row in two parts: its twin for per-row ranges loads `width` and
// `atol` of its row between them and is otherwise this text, so equal inputs give equal bits.
const char* const kRowHead = R"(  const unsigned slot = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (slot >= na) return;  // the whole wave
  const unsigned lane = threadIdx.x & 63u;
  const unsigned row = active[slot];
)";
const char* const kRowRest = R"(  const unsigned s0 = seg_start[row], len = seg_len[row];
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
)";
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

AdaptSweepOptions adapt_sweep_ranges_check(uint64_t rows, int nparams, uint64_t param_count,
                                           const std::vector<double>& a,
                                           const std::vector<double>& b,
                                           const AdaptSweepOptions& opt) {
  const std::string what = "adaptive sweep: ";
  MIINT_CHECK(a.size() == rows && b.size() == rows,
              what + std::to_string(a.size()) + " lower and " + std::to_string(b.size()) +
                  " upper ends for " + std::to_string(rows) + " rows");
  MIINT_CHECK(!opt.unbounded,
              what + "per-row ranges are finite: unbounded takes one shared range");
  // everything but the ends, in adapt_sweep_check's order and words
  const AdaptSweepOptions o = adapt_sweep_check(rows, nparams, param_count, 0.0, 1.0, opt);
  for (uint64_t r = 0; r < rows; ++r)
    MIINT_CHECK(std::isfinite(a[r]) && std::isfinite(b[r]) && std::isfinite(b[r] - a[r]),
                what + "row " + std::to_string(r) + ": a = " + num(a[r]) + " and b = " +
                    num(b[r]) + " must be finite, and b - a too");
  return o;
}

std::string expr_adapt_sweep_ranges_source() {
  return std::string(detail::kRtcPrelude) + R"(
#define MIINT_ROW_WORDS 16ull
#define MIINT_NO_RANK 0xffffffffu
#define MIINT_WAVE_SUM(v) for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64)

// miint_asweep_init with the ends of row r read from lo[r], hi[r]: interval j of row r at
// r * panels + j, edges a + ((b - a) j) / panels, the last one b.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_init_ranges(
    const double* __restrict__ lo_of, const double* __restrict__ hi_of, unsigned rows,
    unsigned panels, double2* __restrict__ list, unsigned* __restrict__ depth,
    unsigned* __restrict__ row, unsigned* __restrict__ active, unsigned* __restrict__ seg_start,
    unsigned* __restrict__ seg_len) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= (unsigned long long)rows * panels) return;
  const unsigned r = (unsigned)(i / panels), j = (unsigned)(i % panels);
  const double a = lo_of[r], b = hi_of[r];
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

// miint_asweep_row with the width and the absolute tolerance of the wave's row read from
// width_of[row], atol_of[row]; the rest is that kernel's text.
extern "C" __global__ __launch_bounds__(256) void miint_asweep_row_ranges(
    unsigned na, const unsigned* __restrict__ active, const unsigned* __restrict__ seg_start,
    const unsigned* __restrict__ seg_len, const double2* __restrict__ list,
    const double* __restrict__ k, const double* __restrict__ err, const double* __restrict__ r,
    const unsigned* __restrict__ depth, const double* __restrict__ width_of, double rtol,
    const double* __restrict__ atol_of, unsigned max_depth, unsigned long long max_intervals,
    unsigned long long round, unsigned long long* __restrict__ st, unsigned* __restrict__ rank,
    unsigned* __restrict__ next_len) {
)" + kRowHead + "  const double width = width_of[row], atol = atol_of[row];\n" + kRowRest + R"(
// The running integral over the m cells' states (miint/expr.hpp, ExprAdaptiveCurve). One
// workgroup. Thread t owns the contiguous run of per = ceil(m / 256) cells from t * per and
// chains their value, err_est, tol and resabs from 0.0 in index order, counting the cells that
// did not converge; thread 0 scans the 256 runs from 0.0 in order and stores the totals; every
// thread then walks its run again and writes point j + 1 = its run's prefix + its chain through
// cell j. out holds four arrays of m + 1 doubles (F, err_est, tol, resabs), bad m + 1 counts.
extern "C" __global__ __launch_bounds__(256) void miint_acurve_prefix(
    unsigned m, int negate, const unsigned long long* __restrict__ st, double* __restrict__ out,
    unsigned* __restrict__ bad, unsigned long long* __restrict__ totals) {
  __shared__ double run[4][256];
  __shared__ unsigned run_bad[256];
  const unsigned per = (m + 255u) / 256u;
  const unsigned first = threadIdx.x * per < m ? threadIdx.x * per : m;
  const unsigned last = first + per < m ? first + per : m;
  const unsigned long long stride = (unsigned long long)m + 1ull;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned nb = 0;
  for (unsigned c = first; c < last; ++c) {
    const unsigned long long* rs = st + MIINT_ROW_WORDS * c;
    const double* rd = (const double*)rs;
    const double v = negate ? -rd[0] : rd[0], e = rd[1], tl = rd[3];
    s[0] += v;
    s[1] += e;
    s[2] += tl;
    s[3] += rd[2];
    nb += (e <= tl && rs[14] == 0ull && rs[12] == 0ull) ? 0u : 1u;
  }
  for (int q = 0; q < 4; ++q) run[q][threadIdx.x] = s[q];
  run_bad[threadIdx.x] = nb;
  __syncthreads();
  if (threadIdx.x == 0) {
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned pb = 0;
    for (int t = 0; t < 256; ++t) {
      for (int q = 0; q < 4; ++q) {
        const double v = run[q][t];
        run[q][t] = p[q];
        p[q] += v;
      }
      const unsigned vb = run_bad[t];
      run_bad[t] = pb;
      pb += vb;
    }
    for (int q = 0; q < 4; ++q) {
      ((double*)totals)[q] = p[q];
      out[stride * q] = 0.0;
    }
    totals[4] = pb;
    bad[0] = 0u;
  }
  __syncthreads();
  double p[4], c4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < 4; ++q) p[q] = run[q][threadIdx.x];
  unsigned pb = run_bad[threadIdx.x];
  for (unsigned c = first; c < last; ++c) {
    const unsigned long long* rs = st + MIINT_ROW_WORDS * c;
    const double* rd = (const double*)rs;
    const double v = negate ? -rd[0] : rd[0], e = rd[1], tl = rd[3];
    c4[0] += v;
    c4[1] += e;
    c4[2] += tl;
    c4[3] += rd[2];
    pb += (e <= tl && rs[14] == 0ull && rs[12] == 0ull) ? 0u : 1u;
    for (int q = 0; q < 4; ++q) out[stride * q + c + 1u] = p[q] + c4[q];
    bad[c + 1u] = pb;
  }
}
)";
}

std::string expr_adapt_sweep_ranges_compile() {
  return detail::rtc_compile_cached(expr_adapt_sweep_ranges_source(), "(per-row ranges)");
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
)" + kRowHead + kRowRest + R"(
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

// lo < hi, opt resolved by adapt_sweep_check. With `ranged` the rows' own ranges and tolerances
// are in ranges_ (upload_ranges; lo and hi are not read) and the two kernels that read them are
// ranged_'s twins.
ExprAdaptiveSweep::Call ExprAdaptiveSweep::rounds(double lo, double hi, uint64_t rows,
                                                  const AdaptSweepOptions& opt, AdaptRange kind,
                                                  double end, bool ranged) {
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
  // ranges_: lo, then hi, width, atol, `rows` doubles each
  const double* lo_of = ranged ? ranges_.get() : nullptr;
  const double* hi_of = ranged ? lo_of + rows : nullptr;
  const double* width_of = ranged ? lo_of + 2 * rows : nullptr;
  const double* atol_of = ranged ? lo_of + 3 * rows : nullptr;
  if (ranged)
    ranged_->launch(kInitRanges, static_cast<unsigned>((n + kBlock - 1) / kBlock), 1, kBlock, s,
                    lo_of, hi_of, k, panels, reinterpret_cast<double2*>(list_[0].get()),
                    depth_[0].get(), row_[0].get(), active_[0].get(), seg_start_.get(),
                    seg_len_.get());
  else
    module_.launch(kInit, static_cast<unsigned>((n + kBlock - 1) / kBlock), 1, kBlock, s, lo, hi,
                   k, panels, reinterpret_cast<double2*>(list_[0].get()), depth_[0].get(),
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
    if (ranged)
      ranged_->launch(kRowRanges, (na32 + kWavesPerBlock - 1) / kWavesPerBlock, 1, kBlock, s, na32,
                      active, static_cast<const unsigned*>(seg_start_.get()),
                      static_cast<const unsigned*>(seg_len_.get()), list,
                      static_cast<const double*>(k_.get()),
                      static_cast<const double*>(err_.get()),
                      static_cast<const double*>(r_.get()), depth, width_of, opt.rtol, atol_of,
                      max_depth, max_iv, round, st, rank_.get(), next_len_.get());
    else
      module_.launch(kRow, (na32 + kWavesPerBlock - 1) / kWavesPerBlock, 1, kBlock, s, na32,
                     active, static_cast<const unsigned*>(seg_start_.get()),
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
  AdaptSweepResult r = zero_rows(rows);
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
  for (uint64_t k = 0; k < rows; ++k) read_row(st.data() + k * kRowWords, swapped, k, &r);
  return r;
}

// Row k of r from the row's sixteen words.
void ExprAdaptiveSweep::read_row(const unsigned long long* w, bool swapped, uint64_t k,
                                 AdaptSweepResult* out) const {
  AdaptSweepResult& r = *out;
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

// ------------------------------------------------------------------ per-row ranges
// The twins that read a row's own range and miint_acurve_prefix: compiled (cached, one source for
// every expression) and loaded once, at the object's first ranged call.
void ExprAdaptiveSweep::load_ranges() {
  if (ranged_) return;
  ranged_.reset(new detail::RtcModule(
      expr_adapt_sweep_ranges_compile(), device_, stream_,
      {"miint_asweep_init_ranges", "miint_asweep_row_ranges", "miint_acurve_prefix"}));
}

std::vector<uint64_t> ExprAdaptiveSweep::upload_ranges(const std::vector<double>& params,
                                                       uint64_t rows,
                                                       const std::vector<double>& a,
                                                       const std::vector<double>& b,
                                                       const double* atol,
                                                       const AdaptSweepOptions& opt) {
  std::vector<uint64_t> live;
  for (uint64_t r = 0; r < rows; ++r)
    if (a[r] != b[r]) live.push_back(r);
  const uint64_t n = live.size();
  if (n == 0) return live;
  reserve(opt.max_total, n);
  if (n > reserved_ranges_) {
    stream_.sync();
    ranges_ = DeviceBuffer<double>(4 * n);
    reserved_ranges_ = n;
  }
  std::vector<double> host(4 * n), p(n * nparams_);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t r = live[i];
    const double lo = std::min(a[r], b[r]), hi = std::max(a[r], b[r]);
    host[i] = lo;
    host[n + i] = hi;
    host[2 * n + i] = hi - lo;  // W of the row, as rounds() forms the shared one
    host[3 * n + i] = atol != nullptr ? atol[r] : opt.atol;
    std::copy(params.begin() + r * nparams_, params.begin() + (r + 1) * nparams_,
              p.begin() + i * nparams_);
  }
  MIINT_HIP(hipMemcpyAsync(ranges_.get(), host.data(), host.size() * sizeof(double),
                           hipMemcpyHostToDevice, stream_.get()));
  stream_.sync();  // host is pageable memory
  upload(p);
  return live;
}

// miint_acurve_prefix's outputs for `points` points: kept across calls like the other buffers.
void ExprAdaptiveSweep::reserve_curve(uint64_t points) {
  if (points > reserved_curve_) {
    stream_.sync();
    curve_ = DeviceBuffer<double>(4 * points);
    curve_bad_ = DeviceBuffer<unsigned>(points);
    reserved_curve_ = points;
  }
  if (curve_totals_.size() == 0) curve_totals_ = PinnedBuffer<unsigned long long>(8);
}

AdaptSweepResult ExprAdaptiveSweep::run_ranges(const std::vector<double>& params, uint64_t rows,
                                               const std::vector<double>& a,
                                               const std::vector<double>& b, const double* atol,
                                               const AdaptSweepOptions& o,
                                               AdaptCurveResult* curve) {
  AdaptSweepResult r = zero_rows(rows);
  for (uint64_t k = 0; k < rows; ++k)
    if (a[k] == b[k]) {  // filled in here; the device never sees the row
      r.tol[k] = atol != nullptr ? atol[k] : o.atol;
      r.converged[k] = 1;
    }
  DeviceGuard g(device_);
  const std::vector<uint64_t> live = upload_ranges(params, rows, a, b, atol, o);
  const uint64_t n = live.size();
  if (n == 0) return r;
  load_ranges();
  const uint64_t points = rows + 1;
  if (curve != nullptr) {
    MIINT_CHECK(n == rows, "adaptive curve: an empty cell");
    reserve_curve(points);
  }
  e0_.record(stream_.get());
  const Call c = rounds(0.0, 0.0, n, o, AdaptRange::kFinite, 0.0, true);
  if (curve != nullptr)
    ranged_->launch(kCurvePrefix, 1, 1, kBlock, stream_.get(), static_cast<unsigned>(rows),
                    a[0] > b[0] ? 1 : 0, static_cast<const unsigned long long*>(state_.get()),
                    curve_.get(), curve_bad_.get(), curve_totals_.device_ptr());
  e1_.record(stream_.get());
  stream_.sync();
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  r.call_rounds = c.rounds;
  r.call_evals = c.evals;
  r.peak = c.peak;
  std::vector<unsigned long long> st(n * kRowWords);
  MIINT_HIP(hipMemcpy(st.data(), state_.get(), st.size() * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < n; ++i)
    read_row(st.data() + i * kRowWords, a[live[i]] > b[live[i]], live[i], &r);
  if (curve != nullptr) {
    std::vector<double> out(4 * points);
    std::vector<unsigned> bad(points);
    MIINT_HIP(hipMemcpy(out.data(), curve_.get(), out.size() * sizeof(double),
                        hipMemcpyDeviceToHost));
    MIINT_HIP(hipMemcpy(bad.data(), curve_bad_.get(), bad.size() * sizeof(unsigned),
                        hipMemcpyDeviceToHost));
    curve->value.assign(out.begin(), out.begin() + points);
    curve->err_est.assign(out.begin() + points, out.begin() + 2 * points);
    curve->tol.assign(out.begin() + 2 * points, out.begin() + 3 * points);
    curve->resabs.assign(out.begin() + 3 * points, out.end());
    curve->converged.resize(points);
    for (uint64_t j = 0; j < points; ++j) curve->converged[j] = bad[j] == 0;
    curve->total = word_as_double(curve_totals_[0]);
    curve->total_err_est = word_as_double(curve_totals_[1]);
    curve->total_tol = word_as_double(curve_totals_[2]);
    curve->total_resabs = word_as_double(curve_totals_[3]);
    curve->unconverged = curve_totals_[4];
  }
  return r;
}

AdaptSweepResult ExprAdaptiveSweep::integrate_ranges(const std::vector<double>& params,
                                                     uint64_t rows, const std::vector<double>& a,
                                                     const std::vector<double>& b,
                                                     const AdaptSweepOptions& opt) {
  const AdaptSweepOptions o =
      adapt_sweep_ranges_check(rows, nparams_, params.size(), a, b, opt);
  return run_ranges(params, rows, a, b, nullptr, o, nullptr);
}

double ExprAdaptiveSweep::time_ranges(const std::vector<double>& params, uint64_t rows,
                                      const std::vector<double>& a, const std::vector<double>& b,
                                      const AdaptSweepOptions& opt, int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive sweep timing request");
  const AdaptSweepOptions o =
      adapt_sweep_ranges_check(rows, nparams_, params.size(), a, b, opt);
  DeviceGuard g(device_);
  const uint64_t n = upload_ranges(params, rows, a, b, nullptr, o).size();
  if (n == 0) return 0.0;
  load_ranges();
  return detail::time_enqueues(stream_, e0_, e1_, iters, [&] {
    (void)rounds(0.0, 0.0, n, o, AdaptRange::kFinite, 0.0, true);
  });
}

// ------------------------------------------------------------------ the running integral
std::vector<double> adapt_curve_atol(const std::vector<double>& x, double atol) {
  std::vector<double> out(x.empty() ? 0 : x.size() - 1);
  const double whole = std::fabs(x.back() - x.front());
  for (size_t c = 0; c < out.size(); ++c) out[c] = (atol * std::fabs(x[c + 1] - x[c])) / whole;
  return out;
}

AdaptSweepOptions adapt_curve_check(const std::vector<double>& x, const AdaptSweepOptions& opt) {
  const std::string what = "adaptive curve: ";
  MIINT_CHECK(x.size() >= 2 && x.size() <= kAdaptCurveMaxCells + 1,
              what + std::to_string(x.size()) + " points: the grid must hold 2..2^20 + 1");
  for (size_t i = 0; i < x.size(); ++i)
    MIINT_CHECK(std::isfinite(x[i]),
                what + "x[" + std::to_string(i) + "] = " + num(x[i]) + " must be finite");
  const bool up = x[1] > x[0];
  for (size_t i = 1; i < x.size(); ++i)
    MIINT_CHECK(up ? x[i] > x[i - 1] : x[i] < x[i - 1],
                what + "x[" + std::to_string(i) + "] = " + num(x[i]) + " after x[" +
                    std::to_string(i - 1) + "] = " + num(x[i - 1]) +
                    ": the grid must be strictly increasing or strictly decreasing");
  MIINT_CHECK(std::isfinite(x.back() - x.front()),
              what + "x[0] = " + num(x.front()) + " and x[M] = " + num(x.back()) +
                  ": x[M] - x[0] must be finite");
  MIINT_CHECK(!opt.unbounded, what + "the grid is finite: unbounded is refused");
  const uint64_t cells = x.size() - 1;
  AdaptSweepOptions o = opt;
  if (o.panels == 0) {
    o.panels = kAdaptDefaultPanels;
    while (o.panels > 1 && cells * o.panels > kAdaptSweepInitialTotal) o.panels >>= 1;
  }
  // max_intervals = 0 becomes max_total / M there, and M * max_intervals <= max_total <= 2^26
  // is checked there
  return adapt_sweep_check(cells, 0, 0, 0.0, 1.0, o);
}

ExprAdaptiveCurve::ExprAdaptiveCurve(const std::string& expr, int device)
    : sweep_(expr, 0, device) {}

AdaptCurveResult ExprAdaptiveCurve::integrate(const std::vector<double>& x,
                                              const AdaptSweepOptions& opt) {
  const AdaptSweepOptions o = adapt_curve_check(x, opt);
  AdaptCurveResult res;
  res.x = x;
  res.atol_cell = adapt_curve_atol(x, o.atol);
  const std::vector<double> a(x.begin(), x.end() - 1), b(x.begin() + 1, x.end());
  res.cells = sweep_.run_ranges({}, a.size(), a, b, res.atol_cell.data(), o, &res);
  res.call_rounds = res.cells.call_rounds;
  res.call_evals = res.cells.call_evals;
  res.peak = res.cells.peak;
  res.device_ms = res.cells.device_ms;
  return res;
}

double ExprAdaptiveCurve::time_prefix(uint64_t cells, int iters) {
  MIINT_CHECK(iters >= 1 && cells >= 1 && cells <= kAdaptCurveMaxCells,
              "bad adaptive curve timing request");
  ExprAdaptiveSweep& s = sweep_;
  DeviceGuard g(s.device_);
  s.reserve(1, cells);
  s.load_ranges();
  s.reserve_curve(cells + 1);
  MIINT_HIP(hipMemsetAsync(s.state_.get(), 0, cells * kRowWords * sizeof(unsigned long long),
                           s.stream_.get()));
  return detail::time_enqueues(s.stream_, s.e0_, s.e1_, iters, [&] {
    s.ranged_->launch(kCurvePrefix, 1, 1, kBlock, s.stream_.get(), static_cast<unsigned>(cells), 0,
                      static_cast<const unsigned long long*>(s.state_.get()), s.curve_.get(),
                      s.curve_bad_.get(), s.curve_totals_.device_ptr());
  });
}

}  // namespace miint
