// Adaptive Gauss-Kronrod (7, 15) integration of a runtime integrand to a requested tolerance
// (see miint/expr.hpp, ExprAdaptive).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kAdaptBlock = 256;
enum { kInit, kEval, kClose, kDecide, kPrefix, kScatter };  // module_'s kernels

// The rule's one table: the non-negative Kronrod nodes from the centre outwards, their
// weights, and the Gauss weights of nodes 0, 2, 4, 6. Hex floats: the correctly rounded
// doubles of the 60-digit values (tests/test_expr_adaptive_cpu.py derives them again).
constexpr double kGkNode[8] = {0x0.0p+0,
                               0x1.a98b2892e0c77p-3,
                               0x1.9f95df119fd62p-2,
                               0x1.2c13a049dfa24p-1,
                               0x1.7ba9f9be3a1d6p-1,
                               0x1.bacf827b9bb3ep-1,
                               0x1.e5f178e7c6229p-1,
                               0x1.fba009d4d09b1p-1};
constexpr double kGkWeight[8] = {0x1.ad04f9087090fp-3,
                                 0x1.a2adbcbec9cd8p-3,
                                 0x1.85d6861c80eb1p-3,
                                 0x1.5a1f266e47d5cp-3,
                                 0x1.200ed0f46e8c1p-3,
                                 0x1.ad384a34814c6p-4,
                                 0x1.026cdaa7b61c4p-4,
                                 0x1.77c5b67d57470p-6};
constexpr double kGaussWeight[4] = {0x1.abfd7e03c2fa6p-2,
                                    0x1.86fe74ee32b3dp-2,
                                    0x1.1e6b1713d8644p-2,
                                    0x1.092f69f826d57p-3};

// The device's totals: words 0..7 are doubles, 8..15 counters. miint_adapt_prefix stores the
// same sixteen words into the pinned record at the end of every round.
enum { kS, kE, kR, kTol, kSumK };
enum { kAccepted = 8, kSplits, kFloor, kForced, kNonfinite, kNext, kCapped, kBase };
constexpr size_t kStateWords = 16;

std::string hex(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%a", v);
  return b;
}

double word_as_double(unsigned long long w) {
  double d;
  std::memcpy(&d, &w, sizeof d);
  return d;
}

std::string num(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.17g", v);
  return b;
}
}  // namespace

std::vector<double> gk15_nodes() {
  std::vector<double> t(15);
  for (int j = 0; j < 8; ++j) {
    t[7 + j] = kGkNode[j];
    t[7 - j] = -kGkNode[j];
  }
  t[7] = 0.0;
  return t;
}

std::vector<double> gk15_weights() {
  std::vector<double> w(15);
  for (int j = 0; j < 8; ++j) w[7 + j] = w[7 - j] = kGkWeight[j];
  return w;
}

std::vector<double> gk7_weights() {
  std::vector<double> w(7);
  for (int j = 0; j < 4; ++j) w[3 + j] = w[3 - j] = kGaussWeight[j];
  return w;
}

void gk15_abscissae(double lo, double hi, double* x15) {
  const double hw = 0.5 * (hi - lo), c = lo + hw;
  x15[7] = c;
  for (int j = 1; j < 8; ++j) {
    x15[7 - j] = std::fma(hw, -kGkNode[j], c);
    x15[7 + j] = std::fma(hw, kGkNode[j], c);
  }
}

const char* adapt_range_name(AdaptRange kind) {
  switch (kind) {
    case AdaptRange::kUpper: return "upper";
    case AdaptRange::kLower: return "lower";
    case AdaptRange::kBoth: return "both";
    default: return "finite";
  }
}

AdaptRange adapt_range(double a, double b) {
  if (std::isnan(a) || std::isnan(b) || a == b) return AdaptRange::kFinite;
  const double lo = std::min(a, b), hi = std::max(a, b);
  if (std::isinf(lo) && std::isinf(hi)) return AdaptRange::kBoth;
  if (std::isinf(hi)) return AdaptRange::kUpper;
  if (std::isinf(lo)) return AdaptRange::kLower;
  return AdaptRange::kFinite;
}

void adapt_range_map(double a, double b, const double* t, uint64_t n, double* x, double* jac,
                     double* x2) {
#pragma clang fp contract(off)  // the device's three lines, each operation rounded on its own
  const AdaptRange kind = adapt_range(a, b);
  MIINT_CHECK(kind != AdaptRange::kBoth || x2 != nullptr,
              "adapt_range_map: the range (-inf, inf) needs the second abscissa x2");
  const double end = std::isinf(a) ? b : a;  // the finite one (unused for kBoth)
  for (uint64_t i = 0; i < n; ++i) {
    if (kind == AdaptRange::kFinite) {
      x[i] = t[i];
      jac[i] = 1.0;
      if (x2 != nullptr) x2[i] = t[i];
      continue;
    }
    const double q = (1.0 - t[i]) / t[i];
    jac[i] = t[i] * t[i];
    if (kind == AdaptRange::kBoth) {
      x[i] = q;
      x2[i] = -q;
    } else {
      x[i] = kind == AdaptRange::kUpper ? end + q : end - q;
      if (x2 != nullptr) x2[i] = x[i];
    }
  }
}

void adapt_check(double a, double b, const AdaptOptions& o) {
  const std::string what = "adaptive: ";
  if (o.unbounded)
    MIINT_CHECK(!std::isnan(a) && !std::isnan(b) &&
                    (std::isinf(a) || std::isinf(b) || std::isfinite(b - a)),
                what + "a = " + num(a) + " and b = " + num(b) +
                    " must not be NaN, and b - a must be finite when both are");
  else
    MIINT_CHECK(std::isfinite(a) && std::isfinite(b) && std::isfinite(b - a),
                what + "a = " + num(a) + " and b = " + num(b) + " must be finite, and b - a too");
  MIINT_CHECK(o.rtol >= 0.0 && o.atol >= 0.0 && std::isfinite(o.rtol) && std::isfinite(o.atol) &&
                  (o.rtol > 0.0 || o.atol > 0.0),
              what + "rtol = " + num(o.rtol) + " and atol = " + num(o.atol) +
                  " must be finite and >= 0, and not both 0");
  MIINT_CHECK(o.max_intervals >= 1 && o.max_intervals <= kAdaptMaxIntervalsLimit,
              what + "max_intervals = " + std::to_string(o.max_intervals) + " must be 1..2^26");
  MIINT_CHECK(o.panels >= 1 && o.panels <= o.max_intervals,
              what + "panels = " + std::to_string(o.panels) + " must be 1..max_intervals = " +
                  std::to_string(o.max_intervals));
  MIINT_CHECK(o.max_depth >= 0 && o.max_depth <= kAdaptMaxDepthLimit,
              what + "max_depth = " + std::to_string(o.max_depth) + " must be 0..200");
}

namespace detail {
std::string adapt_rule_source(const std::string& expr, const std::string& sig,
                              const std::string& args) {
  // the table, printed: the centre, then a pair of nodes per line (the even ones are Gauss nodes)
  std::string rule = "  MIINT_GK_CENTRE(" + hex(kGkWeight[0]) + ", " + hex(kGaussWeight[0]) + ")\n";
  for (int j = 1; j < 8; ++j) {
    if (j % 2 == 0)
      rule += "  MIINT_GK_GAUSS_PAIR(" + hex(kGkNode[j]) + ", " + hex(kGkWeight[j]) + ", " +
              hex(kGaussWeight[j / 2]) + ")\n";
    else
      rule += "  MIINT_GK_PAIR(" + hex(kGkNode[j]) + ", " + hex(kGkWeight[j]) + ")\n";
  }
  return R"(
__device__ __forceinline__ double miint_f(double x)" + sig + R"() { return ()" + expr + R"(); }

// The (7, 15) pair on [lo, hi]: f at the centre and at the seven pairs fma(hw, -+t, c), from
// the centre outwards, the three sums carried by fma in that order.
#define MIINT_GK_CENTRE(wk, wg) \
  { const double f0 = miint_f(c)" + args + R"(); sk = wk * f0; sg = wg * f0; sa = wk * fabs(f0); }
#define MIINT_GK_PAIR(t, wk)                                                  \
  { const double f1 = miint_f(fma(hw, -t, c))" + args + R"(), f2 = miint_f(fma(hw, t, c))" + args + R"();   \
    sk = fma(wk, f1 + f2, sk); sa = fma(wk, fabs(f1) + fabs(f2), sa); }
#define MIINT_GK_GAUSS_PAIR(t, wk, wg)                                        \
  { const double f1 = miint_f(fma(hw, -t, c))" + args + R"(), f2 = miint_f(fma(hw, t, c))" + args + R"();   \
    sk = fma(wk, f1 + f2, sk); sa = fma(wk, fabs(f1) + fabs(f2), sa);         \
    sg = fma(wg, f1 + f2, sg); }
__device__ __forceinline__ void miint_gk15(double lo, double hi)" + sig + R"(, double* k, double* err,
                                           double* r) {
#pragma clang fp contract(off)  // K and G are rounded before they are compared
  const double hw = 0.5 * (hi - lo), c = lo + hw;
  double sk, sg, sa;
)" + rule + R"(  const double kv = hw * sk, gv = hw * sg;
  *k = kv;
  *err = fabs(kv - gv);
  *r = hw * sa;
}
)";
}

std::string adapt_unbounded_rule_source(const std::string& expr, const std::string& sig,
                                        const std::string& args) {
  // the user's f under its own name, compiled as adapt_rule_source compiles it; miint_f becomes
  // g. MIINT_KIND is a literal at every call, so each kernel keeps one branch.
  return R"(
__device__ __forceinline__ double miint_user_f(double x)" + sig + R"() { return ()" + expr + R"(); }

// miint/expr.hpp: q = (1.0 - t) / t, then x, then g, each operation rounded on its own.
// kind 1: (end, +inf); 2: (-inf, end); 3: (-inf, +inf).
__device__ __forceinline__ double miint_g(double t, const int kind, double end)" + sig + R"() {
#pragma clang fp contract(off)
  const double q = (1.0 - t) / t;
  if (kind == 3) return (miint_user_f(q)" + args + R"() + miint_user_f(-q)" + args + R"()) / (t * t);
  const double x = kind == 1 ? end + q : end - q;
  return miint_user_f(x)" + args + R"() / (t * t);
}
)" + adapt_rule_source("miint_g(x, miint_kind, miint_end" + args + ")",
                       ", const int miint_kind, double miint_end" + sig,
                       ", miint_kind, miint_end" + args);
}
}  // namespace detail

std::string expr_adapt_unbounded_source(const std::string& expr) {
  detail::expr_check_named(expr);
  std::string src = std::string(detail::kRtcPrelude) + detail::adapt_unbounded_rule_source(expr, "", "");
  // miint_adapt_eval's twins: the interval is one of t in [0, 1], the block sums and partials
  // are the same.
  const char* names[3] = {"upper", "lower", "both"};
  for (int kind = 1; kind <= 3; ++kind)
    src += std::string(R"(
extern "C" __global__ __launch_bounds__(256) void miint_adapt_eval_)") + names[kind - 1] + R"((
    unsigned long long n, const double2* __restrict__ list, double end, double* __restrict__ k,
    double* __restrict__ err, double* __restrict__ r, double* __restrict__ part_k) {
  __shared__ double red[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    const double2 iv = list[i];
    double e, a;
    miint_gk15(iv.x, iv.y, )" + std::to_string(kind) + R"(, end, &v, &e, &a);
    k[i] = v;
    err[i] = e;
    r[i] = a;
  }
  MIINT_BLOCK_SUM(v, red);
  if (threadIdx.x == 0) part_k[blockIdx.x] = MIINT_RED(red);
}
)";
  return src;
}

std::string expr_adapt_unbounded_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_adapt_unbounded_source(expr), expr);
}

std::string expr_adapt_source(const std::string& expr) {
  detail::expr_check_named(expr);
  return std::string(detail::kRtcPrelude) + detail::adapt_rule_source(expr, "", "") + R"(
// st[0..7] as doubles: S_acc, E_acc, R_acc, tol, sum_K; st[8..15]: accepted, splits, floor,
// forced, nonfinite, next, capped, base (the intervals accepted before this round).
#define MIINT_ST_D(st, i) (((double*)(st))[i])

// The first list: interval i of `panels` equal ones, edges a + ((b - a) i) / panels, the last b.
extern "C" __global__ __launch_bounds__(256) void miint_adapt_init(
    double a, double b, unsigned long long panels, double2* __restrict__ list,
    unsigned* __restrict__ depth) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= panels) return;
  const double w = b - a, p = (double)panels;
  const double lo = a + (w * (double)i) / p;
  const double hi = i + 1 == panels ? b : a + (w * (double)(i + 1)) / p;
  list[i] = make_double2(lo, hi);
  depth[i] = 0u;
}

// One interval per lane: the same fifteen evaluations in every lane, 16-byte endpoint loads.
extern "C" __global__ __launch_bounds__(256) void miint_adapt_eval(
    unsigned long long n, const double2* __restrict__ list, double* __restrict__ k,
    double* __restrict__ err, double* __restrict__ r, double* __restrict__ part_k) {
  __shared__ double red[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    const double2 iv = list[i];
    double e, a;
    miint_gk15(iv.x, iv.y, &v, &e, &a);
    k[i] = v;
    err[i] = e;
    r[i] = a;
  }
  MIINT_BLOCK_SUM(v, red);
  if (threadIdx.x == 0) part_k[blockIdx.x] = MIINT_RED(red);
}

// sum_K over the nb workgroups' partials, then the round's tolerance. A NaN sum gives a NaN
// tolerance (atol > NaN is false).
extern "C" __global__ __launch_bounds__(256) void miint_adapt_close(
    const double* __restrict__ part_k, int nb, double rtol, double atol,
    unsigned long long* __restrict__ st) {
  double sum_k;
  MIINT_CLOSE(part_k, nb, 1.0, sum_k);
  if (threadIdx.x == 0) {
    const double t = rtol * fabs(MIINT_ST_D(st, 0) + sum_k);
    MIINT_ST_D(st, 4) = sum_k;
    MIINT_ST_D(st, 3) = atol > t ? atol : t;
  }
}

// Per interval the decision (miint/expr.hpp has the order); per workgroup the number to split,
// the three counters and five sums: the accepted K, err and R, the K and err to be split.
extern "C" __global__ __launch_bounds__(256) void miint_adapt_decide(
    unsigned long long n, const double2* __restrict__ list, const double* __restrict__ k,
    const double* __restrict__ err, const double* __restrict__ r,
    const unsigned* __restrict__ depth, double width, unsigned max_depth,
    const unsigned long long* __restrict__ st, unsigned char* __restrict__ split,
    unsigned* __restrict__ blk_counts, double* __restrict__ blk_sums) {
  __shared__ double red[5][4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const double tol = ((const double*)st)[3];
  double ak = 0.0, ae = 0.0, ar = 0.0, pk = 0.0, pe = 0.0;
  int how = 0;  // 1 nonfinite, 2 within tolerance, 3 floor, 4 forced, 5 split
  if (i < n) {
    const double2 iv = list[i];
    const double kv = k[i], ev = err[i], rv = r[i];
    const double w = iv.y - iv.x, c = iv.x + 0.5 * w;
    if (!(isfinite(kv) && isfinite(ev))) how = 1;
    else if (!(ev > (tol * w) / width)) how = 2;
    else if (ev <= 0x1.9p-47 * rv) how = 3;  // 50 * 2^-52
    else if (depth[i] >= max_depth || c == iv.x || c == iv.y) how = 4;
    else how = 5;
    split[i] = how == 5 ? 1 : 0;
    if (how == 5) {
      pk = kv;
      pe = ev;
    } else {
      ak = kv;
      ae = ev;
      ar = rv;
    }
  }
  const int n_split = __syncthreads_count(how == 5);
  const int n_floor = __syncthreads_count(how == 3);
  const int n_forced = __syncthreads_count(how == 4);
  const int n_nonfinite = __syncthreads_count(how == 1);
  MIINT_BLOCK_SUM(ak, red[0]);
  MIINT_BLOCK_SUM(ae, red[1]);
  MIINT_BLOCK_SUM(ar, red[2]);
  MIINT_BLOCK_SUM(pk, red[3]);
  MIINT_BLOCK_SUM(pe, red[4]);
  if (threadIdx.x == 0) {
    unsigned* bc = blk_counts + 4ull * blockIdx.x;
    bc[0] = (unsigned)n_split;
    bc[1] = (unsigned)n_floor;
    bc[2] = (unsigned)n_forced;
    bc[3] = (unsigned)n_nonfinite;
    double* bs = blk_sums + 5ull * blockIdx.x;
    for (int q = 0; q < 5; ++q) bs[q] = MIINT_RED(red[q]);
  }
}

// One workgroup over the nb workgroups of the round. Thread t owns the contiguous run of
// per = ceil(nb / 256) of them from t * per: their sums in order, then the block reduction;
// thread 0 scans the 256 runs' split counts, and every thread writes its run's exclusive
// prefixes. Thread 0 then closes the round: capped or not, the totals, the record.
extern "C" __global__ __launch_bounds__(256) void miint_adapt_prefix(
    int nb, unsigned long long n, unsigned long long max_intervals,
    const unsigned* __restrict__ blk_counts, const double* __restrict__ blk_sums,
    unsigned* __restrict__ blk_off, unsigned long long* __restrict__ st,
    unsigned long long* __restrict__ record) {
  __shared__ double red[5][4];
  __shared__ unsigned long long runs[256];
  __shared__ unsigned long long cnt[3][4];
  const int per = (nb + 255) / 256;
  const int first = (int)threadIdx.x * per;
  const int last = first + per < nb ? first + per : nb;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned long long n_split = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int b = first; b < last; ++b) {
    for (int q = 0; q < 5; ++q) s[q] += blk_sums[5ull * b + q];
    n_split += blk_counts[4ull * b];
    c1 += blk_counts[4ull * b + 1];
    c2 += blk_counts[4ull * b + 2];
    c3 += blk_counts[4ull * b + 3];
  }
  runs[threadIdx.x] = n_split;
  for (int o = 32; o > 0; o >>= 1) {
    c1 += __shfl_xor(c1, o, 64);
    c2 += __shfl_xor(c2, o, 64);
    c3 += __shfl_xor(c3, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    cnt[0][threadIdx.x >> 6] = c1;
    cnt[1][threadIdx.x >> 6] = c2;
    cnt[2][threadIdx.x >> 6] = c3;
  }
  MIINT_BLOCK_SUM(s[0], red[0]);
  MIINT_BLOCK_SUM(s[1], red[1]);
  MIINT_BLOCK_SUM(s[2], red[2]);
  MIINT_BLOCK_SUM(s[3], red[3]);
  MIINT_BLOCK_SUM(s[4], red[4]);
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < 256; ++t) {
      const unsigned long long v = runs[t];
      runs[t] = run;
      run += v;
    }
    const unsigned long long accepted = st[8], total_split = run;
    const bool capped = accepted + (n - total_split) + 2ull * total_split > max_intervals;
    st[15] = accepted;
    st[10] += (cnt[0][0] + cnt[0][1]) + (cnt[0][2] + cnt[0][3]);
    st[11] += (cnt[1][0] + cnt[1][1]) + (cnt[1][2] + cnt[1][3]);
    st[12] += (cnt[2][0] + cnt[2][1]) + (cnt[2][2] + cnt[2][3]);
    double rk = MIINT_RED(red[0]), re = MIINT_RED(red[1]);
    if (capped) {  // nothing is split: the pending K and err join the round's sums
      rk += MIINT_RED(red[3]);
      re += MIINT_RED(red[4]);
    }
    MIINT_ST_D(st, 0) += rk;
    MIINT_ST_D(st, 1) += re;
    MIINT_ST_D(st, 2) += MIINT_RED(red[2]);
    st[8] = accepted + (capped ? n : n - total_split);
    st[9] += capped ? 0ull : total_split;
    st[13] = capped ? 0ull : 2ull * total_split;
    st[14] = capped ? 1ull : 0ull;
    for (int q = 0; q < 8; ++q) MIINT_ST_D(record, q) = MIINT_ST_D(st, q);
    for (int q = 8; q < 16; ++q) record[q] = st[q];
  }
  __syncthreads();
  unsigned long long off = runs[threadIdx.x];
  for (int b = first; b < last; ++b) {
    blk_off[b] = (unsigned)off;
    off += blk_counts[4ull * b];
  }
}

// Children (lo, c), (c, hi) at depth + 1 to slots 2 p, 2 p + 1 of the next list, p the number
// of intervals split before this one: blk_off plus the lanes before it in the workgroup
// (ballot and popcount per wave, the waves' counts through LDS). An accepted interval (all of
// them in a capped round) goes to slot base + (the accepted before it) of `done`, if given.
// Nothing is stored at or past next_cap or done_cap.
extern "C" __global__ __launch_bounds__(256) void miint_adapt_scatter(
    unsigned long long n, const double2* __restrict__ list, const unsigned* __restrict__ depth,
    const unsigned char* __restrict__ split, const unsigned* __restrict__ blk_off,
    const unsigned long long* __restrict__ st, double2* __restrict__ next,
    unsigned* __restrict__ next_depth, unsigned long long next_cap, double2* __restrict__ done,
    unsigned long long done_cap) {
  __shared__ unsigned waves[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool capped = st[14] != 0ull;
  const bool valid = i < n;
  const bool sp = valid && !capped && split[i] != 0;
  const unsigned long long mask = __ballot(sp);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) waves[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  unsigned before = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  for (unsigned w = 0; w < wave; ++w) before += waves[w];
  if (!valid) return;
  const double2 iv = list[i];
  const unsigned long long p = capped ? 0ull : (unsigned long long)blk_off[blockIdx.x] + before;
  if (sp) {
    const double c = iv.x + 0.5 * (iv.y - iv.x);
    const unsigned d = depth[i] + 1u;
    if (2ull * p + 1ull < next_cap) {
      next[2ull * p] = make_double2(iv.x, c);
      next[2ull * p + 1ull] = make_double2(c, iv.y);
      next_depth[2ull * p] = d;
      next_depth[2ull * p + 1ull] = d;
    }
  } else if (done != nullptr) {
    const unsigned long long q = st[15] + (i - p);
    if (q < done_cap) done[q] = iv;
  }
}
)";
}

std::string expr_adapt_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_adapt_source(expr), expr);
}

ExprAdaptive::ExprAdaptive(const std::string& expr, int device)
    : expr_(expr), device_(device), stream_((set_device(device), Stream())),
      module_(expr_adapt_compile(expr), device, stream_,
              {"miint_adapt_init", "miint_adapt_eval", "miint_adapt_close", "miint_adapt_decide",
               "miint_adapt_prefix", "miint_adapt_scatter"}) {
  DeviceGuard g(device);
  state_ = DeviceBuffer<unsigned long long>(kStateWords);
  record_ = PinnedBuffer<unsigned long long>(kStateWords);
}

// The eval kernels of the infinite kinds: compiled (cached per expression) and loaded once, at
// the object's first unbounded call.
void ExprAdaptive::load_unbounded() {
  if (unbounded_) return;
  unbounded_.reset(new detail::RtcModule(
      expr_adapt_unbounded_compile(expr_), device_, stream_,
      {"miint_adapt_eval_upper", "miint_adapt_eval_lower", "miint_adapt_eval_both"}));
}

// Every buffer holds max_intervals intervals (or their workgroups): sized once for the
// largest max_intervals asked so far and kept across calls.
void ExprAdaptive::reserve(uint64_t m) {
  if (m <= reserved_) return;
  stream_.sync();
  const uint64_t nb = (m + kAdaptBlock - 1) / kAdaptBlock;
  for (int q = 0; q < 2; ++q) {
    list_[q] = DeviceBuffer<double>(2 * m);
    depth_[q] = DeviceBuffer<unsigned>(m);
  }
  k_ = DeviceBuffer<double>(m);
  err_ = DeviceBuffer<double>(m);
  r_ = DeviceBuffer<double>(m);
  split_ = DeviceBuffer<unsigned char>(m);
  part_k_ = DeviceBuffer<double>(nb);
  blk_sums_ = DeviceBuffer<double>(5 * nb);
  blk_counts_ = DeviceBuffer<unsigned>(4 * nb);
  blk_off_ = DeviceBuffer<unsigned>(nb);
  reserved_ = m;
}

// lo < hi. `out` (or null) takes the partition in acceptance order; integrate() orders it.
AdaptResult ExprAdaptive::rounds(double lo, double hi, const AdaptOptions& opt, double* out,
                                 uint64_t cap, AdaptRange kind, double end,
                                 const EvalTwin* twin) {
  hipStream_t s = stream_.get();
  const unsigned long long max_iv = opt.max_intervals;
  const unsigned max_depth = static_cast<unsigned>(opt.max_depth);
  const double width = hi - lo;
  double2* done = reinterpret_cast<double2*>(out);
  const unsigned long long done_cap = cap;
  unsigned long long* st = state_.get();
  unsigned long long* rec = record_.device_ptr();
  MIINT_HIP(hipMemsetAsync(st, 0, kStateWords * sizeof(unsigned long long), s));
  unsigned long long n = opt.panels;
  int cur = 0;
  module_.launch(kInit, static_cast<unsigned>((n + kAdaptBlock - 1) / kAdaptBlock), 1, kAdaptBlock,
                 s, lo, hi, n, reinterpret_cast<double2*>(list_[0].get()), depth_[0].get());
  AdaptResult r;
  for (;;) {
    MIINT_CHECK(n >= 1 && n <= max_iv && n <= reserved_, "adaptive: the active list left its bound");
    MIINT_CHECK(r.rounds <= static_cast<uint64_t>(opt.max_depth), "adaptive: more rounds than depths");
    const unsigned blocks = static_cast<unsigned>((n + kAdaptBlock - 1) / kAdaptBlock);
    const int nb = static_cast<int>(blocks);
    const double2* list = reinterpret_cast<const double2*>(list_[cur].get());
    double2* next = reinterpret_cast<double2*>(list_[cur ^ 1].get());
    const unsigned* depth = depth_[cur].get();
    if (twin != nullptr)
      twin->launch(blocks, n, list_[cur].get(), depth);
    else if (kind == AdaptRange::kFinite)
      module_.launch(kEval, blocks, 1, kAdaptBlock, s, n, list, k_.get(), err_.get(), r_.get(),
                     part_k_.get());
    else  // the twin of the kind: kernels 0, 1, 2 of unbounded_
      unbounded_->launch(static_cast<size_t>(kind) - 1, blocks, 1, kAdaptBlock, s, n, list, end,
                         k_.get(), err_.get(), r_.get(), part_k_.get());
    module_.launch(kClose, 1, 1, kAdaptBlock, s, static_cast<const double*>(part_k_.get()), nb,
                   opt.rtol, opt.atol, st);
    module_.launch(kDecide, blocks, 1, kAdaptBlock, s, n, list,
                   static_cast<const double*>(k_.get()), static_cast<const double*>(err_.get()),
                   static_cast<const double*>(r_.get()), depth, width, max_depth,
                   static_cast<const unsigned long long*>(st), split_.get(), blk_counts_.get(),
                   blk_sums_.get());
    module_.launch(kPrefix, 1, 1, kAdaptBlock, s, nb, n, max_iv,
                   static_cast<const unsigned*>(blk_counts_.get()),
                   static_cast<const double*>(blk_sums_.get()), blk_off_.get(), st, rec);
    module_.launch(kScatter, blocks, 1, kAdaptBlock, s, n, list, depth,
                   static_cast<const unsigned char*>(split_.get()),
                   static_cast<const unsigned*>(blk_off_.get()),
                   static_cast<const unsigned long long*>(st), next, depth_[cur ^ 1].get(), max_iv,
                   done, done_cap);
    stream_.sync();
    ++r.rounds;
    r.evals += (twin != nullptr ? twin->evals_per : 15) * n;
    if (record_[kCapped] != 0 || record_[kNext] == 0) break;
    n = record_[kNext];
    cur ^= 1;
  }
  r.value = word_as_double(record_[kS]);
  r.err_est = word_as_double(record_[kE]);
  r.resabs = word_as_double(record_[kR]);
  r.tol = word_as_double(record_[kTol]);
  r.intervals = record_[kAccepted];
  r.splits = record_[kSplits];
  r.floor = record_[kFloor];
  r.forced = record_[kForced];
  r.nonfinite = record_[kNonfinite];
  r.capped = record_[kCapped] != 0;
  r.converged = r.err_est <= r.tol && !r.capped && r.nonfinite == 0;
  return r;
}

AdaptResult ExprAdaptive::integrate(double a, double b, const AdaptOptions& opt,
                                    double* intervals_out, uint64_t capacity) {
  adapt_check(a, b, opt);
  MIINT_CHECK(intervals_out == nullptr || capacity >= opt.max_intervals,
              "adaptive: intervals_out holds " + std::to_string(capacity) +
                  " intervals, fewer than max_intervals = " + std::to_string(opt.max_intervals));
  if (a == b) {
    AdaptResult r;
    r.tol = opt.atol;
    r.converged = true;
    return r;
  }
  DeviceGuard g(device_);
  reserve(opt.max_intervals);
  const bool swapped = a > b;
  const AdaptRange kind = adapt_range(a, b);
  const bool mapped = kind != AdaptRange::kFinite;
  if (mapped) load_unbounded();
  const double end = std::isinf(a) ? b : a;  // the finite end of a half-infinite range
  e0_.record(stream_.get());
  AdaptResult r = mapped ? rounds(0.0, 1.0, opt, intervals_out, capacity, kind, end)
                         : rounds(swapped ? b : a, swapped ? a : b, opt, intervals_out, capacity);
  e1_.record(stream_.get());
  stream_.sync();
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  r.range = adapt_range_name(kind);
  if (swapped) r.value = -r.value;
  if (intervals_out != nullptr) {
    // the rounds stored the partition in acceptance order: the intervals are disjoint, so the
    // order of their lower ends is the x order. Not on the rounds' path: ordered on the host.
    MIINT_CHECK(r.intervals <= capacity, "adaptive: the partition passed intervals_out");
    std::vector<std::pair<double, double>> iv(r.intervals);
    MIINT_HIP(hipMemcpy(iv.data(), intervals_out, iv.size() * 2 * sizeof(double),
                        hipMemcpyDeviceToHost));
    std::sort(iv.begin(), iv.end());
    if (swapped && !mapped) {  // from a down to b; a mapped range stays ascending in t
      std::reverse(iv.begin(), iv.end());
      for (auto& p : iv) std::swap(p.first, p.second);
    }
    MIINT_HIP(hipMemcpy(intervals_out, iv.data(), iv.size() * 2 * sizeof(double),
                        hipMemcpyHostToDevice));
  }
  return r;
}

double ExprAdaptive::time(double a, double b, const AdaptOptions& opt, int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive timing request");
  adapt_check(a, b, opt);
  if (a == b) return 0.0;
  DeviceGuard g(device_);
  reserve(opt.max_intervals);
  const AdaptRange kind = adapt_range(a, b);
  if (kind != AdaptRange::kFinite) {
    load_unbounded();
    const double end = std::isinf(a) ? b : a;
    return detail::time_enqueues(stream_, e0_, e1_, iters,
                                 [&] { (void)rounds(0.0, 1.0, opt, nullptr, 0, kind, end); });
  }
  const double lo = std::min(a, b), hi = std::max(a, b);
  return detail::time_enqueues(stream_, e0_, e1_, iters,
                               [&] { (void)rounds(lo, hi, opt, nullptr, 0); });
}

}  // namespace miint
