// Adaptive Filon-Clenshaw-Curtis (13, 25) integration of a runtime f(x) against cos(omega x) or
// sin(omega x) to a requested tolerance, and the Fourier tail on (a, +inf): the rounds of
// intervals (detail::AdaptRounds) around another evaluation kernel (see miint/expr.hpp,
// ExprAdaptiveOsc).
#include <algorithm>
#include <cmath>
#include <complex>
#include <limits>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kOscBlock = 256;
constexpr int kN = 24;  // the fine rule's degree; the coarse one's is kN / 2

// t_j = cos(j pi / 24), j = 0 .. 12, and the Clenshaw-Curtis weights of those nodes: the
// correctly rounded doubles of the 60-digit values (tests/test_expr_osc_cpu.py derives them
// again). t_12 is 0.
constexpr double kOscNode[13] = {0x1.0000000000000p+0,
                                 0x1.fb9ea92ec689bp-1,
                                 0x1.ee8dd4748bf15p-1,
                                 0x1.d906bcf328d46p-1,
                                 0x1.bb67ae8584caap-1,
                                 0x1.963268b572492p-1,
                                 0x1.6a09e667f3bcdp-1,
                                 0x1.37af93f9513eap-1,
                                 0x1.0000000000000p-1,
                                 0x1.87de2a6aea963p-2,
                                 0x1.0907dc1930690p-2,
                                 0x1.0b5150f6da2d1p-3,
                                 0x0.0p+0};
constexpr double kCcWeight[13] = {0x1.c7e7115d0ce95p-10,
                                  0x1.1136155e7fab0p-6,
                                  0x1.16bd58d300657p-5,
                                  0x1.99c110b8e71e5p-5,
                                  0x1.0c44dafeb6b01p-4,
                                  0x1.46449f78293b1p-4,
                                  0x1.7b38f95df064dp-4,
                                  0x1.a94a8680bc943p-4,
                                  0x1.d065d7f1c74a7p-4,
                                  0x1.ef4b6714c6798p-4,
                                  0x1.02f96654f0e63p-3,
                                  0x1.09c399b07d2b9p-3,
                                  0x1.0c1b703601543p-3};

using ld = long double;
constexpr ld kPi = 3.14159265358979323846264338327950288L;
constexpr ld kBesselBelow = 64.0L;  // |par| below this: the Bessel series; else forwards

using detail::hex;
using detail::num;

// int_{-1}^{1} T_k T_n dt
ld cheb_pair(int k, int n) {
  if ((k + n) % 2 != 0) return 0.0L;
  const ld s = static_cast<ld>(k + n), d = static_cast<ld>(k - n);
  return 1.0L / (1.0L - s * s) + 1.0L / (1.0L - d * d);
}

// The moments of miint/expr.hpp for th >= 0: mc[k] = int T_k cos(th t) (k even, else 0),
// ms[k] = int T_k sin(th t) (k odd, else 0), k = 0 .. 24.
void moments(ld th, ld* mc, ld* ms) {
  for (int k = 0; k <= kN; ++k) mc[k] = ms[k] = 0.0L;
  if (th == 0.0L) {
    for (int k = 0; k <= kN; k += 2) mc[k] = 2.0L / (1.0L - static_cast<ld>(k) * k);
    return;
  }
  if (th < kBesselBelow) {
    const int top = 2 * static_cast<int>(std::ceil(static_cast<double>(th) / 2.0)) + 96;
    std::vector<ld> j(top + 2, 0.0L);
    j[top] = 1e-2000L;
    for (int n = top; n >= 1; --n) {
      j[n - 1] = (2.0L * n / th) * j[n] - j[n + 1];
      if (std::fabs(j[n - 1]) > 1e2000L)  // keep the unnormalised run in range
        for (int q = n - 1; q <= top; ++q) j[q] *= 1e-2000L;
    }
    ld norm = j[0];
    for (int m = 2; m <= top; m += 2) norm += 2.0L * j[m];
    for (int n = 0; n <= top; ++n) j[n] /= norm;
    for (int k = 0; k <= kN; ++k) {
      ld sum = 0.0L;
      for (int n = k % 2; n <= top; n += 2) {
        const ld eps = n == 0 ? 1.0L : 2.0L;
        const ld sign = ((n / 2) % 2 == 0) ? 1.0L : -1.0L;  // i^n, or i^(n - 1) for odd n
        sum += eps * sign * j[n] * cheb_pair(k, n);
      }
      (k % 2 == 0 ? mc : ms)[k] = sum;
    }
    return;
  }
  using cld = std::complex<ld>;
  const ld s = std::sin(th), c = std::cos(th);
  const cld ith(0.0L, th);
  const cld b_even(0.0L, 2.0L * s), b_odd(2.0L * c, 0.0L);  // exp(i th) -+ exp(-i th)
  cld m[kN + 1], d[kN + 1];
  m[0] = cld(2.0L * s / th, 0.0L);
  d[0] = cld(0.0L, 0.0L);
  d[1] = m[0];
  m[1] = (b_odd - d[1]) / ith;
  d[2] = 4.0L * m[1];
  m[2] = (b_even - d[2]) / ith;
  for (int k = 2; k < kN; ++k) {
    d[k + 1] = static_cast<ld>(k + 1) * (2.0L * m[k] + d[k - 1] / static_cast<ld>(k - 1));
    m[k + 1] = (((k + 1) % 2 == 0 ? b_even : b_odd) - d[k + 1]) / ith;
  }
  for (int k = 0; k <= kN; ++k) (k % 2 == 0 ? mc : ms)[k] = k % 2 == 0 ? m[k].real() : m[k].imag();
}

// cos(m pi / n) for integers, the argument reduced exactly.
ld cos_pi_ratio(long m, long n) {
  m %= 2 * n;
  if (m > n) m = 2 * n - m;
  if (2 * m == n) return 0.0L;
  if (2 * m > n) return -std::cos(kPi * static_cast<ld>(n - m) / static_cast<ld>(n));
  return std::cos(kPi * static_cast<ld>(m) / static_cast<ld>(n));
}

// The weights of the (n + 1)-node rule for j = 0 .. n / 2 from the moments.
void half_weights(int n, const ld* mc, const ld* ms, double* wc, double* ws) {
  for (int j = 0; j <= n / 2; ++j) {
    ld sc = 0.0L, ss = 0.0L;
    for (int k = 0; k <= n; ++k) {
      const ld half = (k == 0 || k == n) ? 0.5L : 1.0L;
      const ld ck = cos_pi_ratio(static_cast<long>(j) * k, n);
      sc += half * ck * mc[k];
      ss += half * ck * ms[k];
    }
    const ld scale = (2.0L / n) * (j == 0 ? 0.5L : 1.0L);
    wc[j] = static_cast<double>(scale * sc);
    ws[j] = j == n / 2 ? 0.0 : static_cast<double>(scale * ss);
  }
}

struct HalfTables {
  double wc24[13], ws24[13], wc12[7], ws12[7];
};

HalfTables half_tables(double par) {
  MIINT_CHECK(std::isfinite(par), "osc_weights: par = " + num(par) + " must be finite");
  ld mc[kN + 1], ms[kN + 1];
  moments(std::fabs(static_cast<ld>(par)), mc, ms);
  HalfTables h;
  half_weights(kN, mc, ms, h.wc24, h.ws24);
  half_weights(kN / 2, mc, ms, h.wc12, h.ws12);
  if (par < 0.0) {  // sin is odd in par
    for (double& v : h.ws24) v = -v;
    for (double& v : h.ws12) v = -v;
  }
  for (double& v : h.ws24) v += 0.0;  // no negative zeros in the table
  for (double& v : h.ws12) v += 0.0;
  return h;
}
}  // namespace

const char* osc_kind_name(OscKind kind) { return kind == OscKind::kSin ? "sin" : "cos"; }

OscKind osc_kind(const std::string& name) {
  if (name == "cos") return OscKind::kCos;
  if (name == "sin") return OscKind::kSin;
  fail("oscillatory: kind '" + name + "' must be cos or sin", __FILE__, __LINE__);
  return OscKind::kCos;
}

std::vector<double> osc_nodes() {
  std::vector<double> t(25);
  for (int j = 0; j <= 12; ++j) {
    t[j] = kOscNode[j];
    t[24 - j] = -kOscNode[j];
  }
  t[12] = 0.0;
  return t;
}

std::vector<double> osc_cc_weights() {
  std::vector<double> w(25);
  for (int j = 0; j <= 12; ++j) w[j] = w[24 - j] = kCcWeight[j];
  return w;
}

std::vector<double> osc_weights(double par) {
  const HalfTables h = half_tables(par);
  std::vector<double> w(76);
  for (int j = 0; j <= 12; ++j) {
    w[j] = w[24 - j] = h.wc24[j];
    w[25 + j] = h.ws24[j];
    w[25 + 24 - j] = 0.0 - h.ws24[j];
  }
  for (int j = 0; j <= 6; ++j) {
    w[50 + j] = w[50 + 12 - j] = h.wc12[j];
    w[63 + j] = h.ws12[j];
    w[63 + 12 - j] = 0.0 - h.ws12[j];
  }
  return w;
}

void osc_table_row(double par, double* row) {
  const HalfTables h = half_tables(par);
  for (int j = 0; j <= 12; ++j) row[j] = h.wc24[j];
  for (int j = 0; j <= 11; ++j) row[13 + j] = h.ws24[j];
  for (int j = 0; j <= 6; ++j) row[25 + j] = h.wc12[j];
  for (int j = 0; j <= 5; ++j) row[32 + j] = h.ws12[j];
  row[38] = row[39] = 0.0;
}

void osc_abscissae(double lo, double hi, double* x25) {
  const double hw = 0.5 * (hi - lo), c = lo + hw;
  x25[12] = c;
  for (int j = 0; j < 12; ++j) {
    x25[j] = std::fma(hw, kOscNode[j], c);
    x25[24 - j] = std::fma(hw, -kOscNode[j], c);
  }
}

void osc_check(double a, double b, double omega, const AdaptOptions& opt, bool tail,
               const OscTailOptions& topt) {
  const std::string what = "oscillatory: ";
  MIINT_CHECK(std::isfinite(omega), what + "omega = " + num(omega) + " must be finite");
  MIINT_CHECK(!(std::isinf(a) && a < 0.0) && !(std::isinf(b) && b < 0.0) &&
                  !(std::isinf(a) && a > 0.0),
              what + "a = " + num(a) + ", b = " + num(b) +
                  ": only (a, +inf) with a finite is supported among the infinite ranges "
                  "((-inf, b) and two-sided Fourier integrals are not)");
  if (!tail) {
    MIINT_CHECK(!std::isinf(b), what + "b = inf is the Fourier tail: call integrate_tail");
    AdaptOptions o = opt;
    o.unbounded = false;
    adapt_check(a, b, o);
    return;
  }
  MIINT_CHECK(std::isfinite(a) && std::isinf(b) && b > 0.0,
              what + "the Fourier tail runs on (a, +inf) with a finite: a = " + num(a) +
                  ", b = " + num(b));
  MIINT_CHECK(omega != 0.0, what + "omega = 0 with an infinite end is not supported (that is "
                                   "the unbounded adaptive rule's integral)");
  MIINT_CHECK(opt.atol > 0.0 && std::isfinite(opt.atol),
              what + "the Fourier tail needs atol > 0 (atol = " + num(opt.atol) +
                  "): the cycles are held to shares of an absolute tolerance, rtol alone is "
                  "refused");
  MIINT_CHECK(topt.max_cycles >= 1 && topt.max_cycles <= 10000,
              what + "max_cycles = " + std::to_string(topt.max_cycles) + " must be 1..10000");
  AdaptOptions o = opt;
  o.unbounded = false;
  o.rtol = 0.0;
  o.panels = topt.panels;
  adapt_check(a, a + 1.0, o);
}

std::string expr_osc_source(const std::string& expr) {
  detail::expr_check_named(expr);
  // the pairs, printed from the outermost but one inwards order of the header: j = 11 .. 0
  std::string rule;
  for (int j = 11; j >= 0; --j) {
    const char* macro = j == 11 ? "MIINT_OSC_FIRST" : j == 10 ? "MIINT_OSC_FIRST_EVEN"
                        : j % 2 == 0 ? "MIINT_OSC_EVEN" : "MIINT_OSC_ODD";
    rule += std::string("  ") + macro + "(" + std::to_string(j) + ", " + hex(kOscNode[j]) + ", " +
            hex(kCcWeight[j]) + ")\n";
  }
  const std::string body = R"(
__device__ __forceinline__ double miint_f(double x) { (void)x; return ()" + expr + R"(); }

// A depth's row of the weight table: Wc24 at 0..12 (12 the centre), Ws24 at 13..24, Wc12 at
// 25..31 (node 2 m at 25 + m), Ws12 at 32..37.
#define MIINT_OSC_VALUES(t)                                                     \
  const double fp = miint_f(fma(hw, t, c)), fm = miint_f(fma(hw, -t, c));       \
  const double s = fp + fm, d = fp - fm;
#define MIINT_OSC_FIRST(j, t, w)                                                \
  { MIINT_OSC_VALUES(t)                                                         \
    ic24 = fma(row[j], s, ic24); is24 = row[13 + j] * d;                        \
    sa = fma(w, fabs(fp) + fabs(fm), sa); }
#define MIINT_OSC_FIRST_EVEN(j, t, w)                                           \
  { MIINT_OSC_VALUES(t)                                                         \
    ic24 = fma(row[j], s, ic24); is24 = fma(row[13 + j], d, is24);              \
    ic12 = fma(row[25 + j / 2], s, ic12); is12 = row[32 + j / 2] * d;           \
    sa = fma(w, fabs(fp) + fabs(fm), sa); }
#define MIINT_OSC_ODD(j, t, w)                                                  \
  { MIINT_OSC_VALUES(t)                                                         \
    ic24 = fma(row[j], s, ic24); is24 = fma(row[13 + j], d, is24);              \
    sa = fma(w, fabs(fp) + fabs(fm), sa); }
#define MIINT_OSC_EVEN(j, t, w)                                                 \
  { MIINT_OSC_VALUES(t)                                                         \
    ic24 = fma(row[j], s, ic24); is24 = fma(row[13 + j], d, is24);              \
    ic12 = fma(row[25 + j / 2], s, ic12); is12 = fma(row[32 + j / 2], d, is12); \
    sa = fma(w, fabs(fp) + fabs(fm), sa); }

// Filon-Clenshaw-Curtis (13, 25) on [lo, hi] (miint/expr.hpp): the centre, then the mirrored
// pairs from the centre outwards, the five sums carried by fma in that order; the weight's
// phase at the centre. kind 0: cos(omega x), 1: sin(omega x).
__device__ __forceinline__ void miint_osc_rule(double lo, double hi, const double* __restrict__ row,
                                               double omega, const int kind, double* k,
                                               double* err, double* r) {
#pragma clang fp contract(off)  // K and G are rounded before they are compared
  const double hw = 0.5 * (hi - lo), c = lo + hw;
  const double f12 = miint_f(c);
  double ic24 = row[12] * f12, ic12 = row[31] * f12, is24, is12;
  double sa = )" + hex(kCcWeight[12]) + R"( * fabs(f12);
)" + rule + R"(  const double p = omega * c, e = fma(omega, c, -p);
  double s0, c0;
  sincos(p, &s0, &c0);
  const double sn = fma(e, c0, s0), cs = fma(-e, s0, c0);
  double kv, gv;
  if (kind == 0) {
    kv = hw * (cs * ic24 - sn * is24);
    gv = hw * (cs * ic12 - sn * is12);
  } else {
    kv = hw * (sn * ic24 + cs * is24);
    gv = hw * (sn * ic12 + cs * is12);
  }
  *k = kv;
  *err = fabs(kv - gv);
  *r = hw * sa;
}
)";
  std::string src = std::string(detail::kRtcPrelude) + body;
  // miint_adapt_eval's twins: the interval's depth picks the row (never past rows - 1), the
  // block sums and partials are the same.
  const char* names[2] = {"cos", "sin"};
  for (int kind = 0; kind < 2; ++kind)
    src += "\n" + detail::adapt_eval_source(
        "", std::string("miint_osc_eval_") + names[kind],
        R"(unsigned long long n, const double2* __restrict__ list, const unsigned* __restrict__ depth,
    const double* __restrict__ table, unsigned rows, double omega, double* __restrict__ k,
    double* __restrict__ err, double* __restrict__ r, double* __restrict__ part_k)",
        "    const double2 iv = list[i];\n"
        "    const unsigned d = depth[i] < rows ? depth[i] : rows - 1u;\n    double e, a;\n"
        "    miint_osc_rule(iv.x, iv.y, table + " + std::to_string(kOscRow) + "ull * d, omega, " +
            std::to_string(kind) + ", &v, &e, &a);\n");
  return src;
}

std::string expr_osc_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_osc_source(expr), expr);
}

double osc_epsilon(const double* s, int n) {
#pragma clang fp contract(off)
  MIINT_CHECK(n >= 3, "osc_epsilon: at least 3 partial sums");
  std::vector<double> before(n + 1, 0.0), prev(s, s + n), cur(n);
  double best = s[n - 1];
  for (int col = 1; col < n; ++col) {
    const int len = n - col;
    bool ok = true;
    for (int i = 0; i < len && ok; ++i) {
      const double diff = prev[i + 1] - prev[i];
      if (diff == 0.0 || !std::isfinite(diff)) ok = false;
      else cur[i] = before[i + 1] + 1.0 / diff;
    }
    if (!ok) break;
    if (col % 2 == 0) {
      if (!std::isfinite(cur[len - 1])) break;
      best = cur[len - 1];
    }
    for (int i = 0; i < len + 1; ++i) before[i] = prev[i];
    for (int i = 0; i < len; ++i) prev[i] = cur[i];
  }
  return best;
}

std::string osc_reason(const AdaptResult& r) {
  if (r.converged) return "";
  if (r.nonfinite != 0)
    return "f was not finite on " + std::to_string(r.nonfinite) +
           " intervals (both ends of every interval are evaluated)";
  if (r.capped) return "max_intervals was reached";
  if (r.forced != 0)
    return std::to_string(r.forced) + " intervals reached max_depth or could not be halved";
  return "the rounding floor was reached on " + std::to_string(r.floor) +
         " intervals before the tolerance";
}

ExprAdaptiveOsc::ExprAdaptiveOsc(const std::string& expr, int device)
    : expr_(expr), rounds_(1, expr_adapt_compile(expr), "miint_adapt_eval", device),
      twins_(expr_osc_compile(expr), device, rounds_.stream(),
             {"miint_osc_eval_cos", "miint_osc_eval_sin"}) {}

// Rows 0 .. upto of the table for par0 on the device: a row is computed and sent when the
// first round that can hold its depth is about to be enqueued.
void ExprAdaptiveOsc::upload(double par0, int rows, int upto) {
  if (static_cast<int>(host_table_.size()) < rows * kOscRow || table_rows_ < rows) {
    rounds_.stream().sync();
    host_table_.assign(static_cast<size_t>(rows) * kOscRow, 0.0);
    table_ = DeviceBuffer<double>(static_cast<size_t>(rows) * kOscRow);
    table_rows_ = rows;
    table_depths_ = 0;
  }
  if (table_depths_ == 0 || par0 != table_par0_) {
    table_par0_ = par0;
    table_depths_ = 0;
    ++uploads_;
  }
  upto = std::min(upto, rows - 1);
  for (int d = table_depths_; d <= upto; ++d) {
    double* row = host_table_.data() + static_cast<size_t>(d) * kOscRow;
    osc_table_row(std::ldexp(par0, -d), row);
    MIINT_HIP(hipMemcpyAsync(table_.get() + static_cast<size_t>(d) * kOscRow, row,
                             kOscRow * sizeof(double), hipMemcpyHostToDevice,
                             rounds_.stream().get()));
    table_depths_ = d + 1;
  }
}

// The rounds of `job` around the twin of `kind`; hw0 is the nominal half width of a first
// interval. `timed`: between the events, the partition ordered (AdaptRounds::integrate).
AdaptResult ExprAdaptiveOsc::run(const detail::AdaptJob& job, double hw0, double omega,
                                 OscKind kind, bool timed) {
  const double par0 = omega * hw0;
  const int rows = job.max_depth + 1;
  int round = 0;
  const detail::AdaptRounds::Eval eval = [&](const detail::AdaptItems& it) {
    upload(par0, rows, round++);  // round t holds depths 0 .. t
    twins_.launch(static_cast<size_t>(kind), it.blocks, 1, kOscBlock, it.stream, it.n, it.xs,
                  it.depth, static_cast<const double*>(table_.get()), static_cast<unsigned>(rows),
                  omega, it.k, it.err, it.r, it.part_k);
  };
  return timed ? rounds_.integrate<AdaptResult>(job, 25, eval)
               : rounds_.run<AdaptResult>(job, 25, eval);
}

OscResult ExprAdaptiveOsc::integrate(double a, double b, double omega, OscKind kind,
                                     const AdaptOptions& opt, double* intervals_out,
                                     uint64_t capacity) {
  if (std::isinf(b) && b > 0.0 && std::isfinite(a)) {
    MIINT_CHECK(intervals_out == nullptr,
                "oscillatory: the Fourier tail returns no partition (intervals_out)");
    return integrate_tail(a, omega, kind, opt);
  }
  osc_check(a, b, omega, opt);
  rounds_.check_capacity(intervals_out, capacity, opt.max_intervals);
  OscResult res;
  res.omega = omega;
  res.kind = osc_kind_name(kind);
  if (a == b) {
    res.tol = opt.atol;
    res.converged = true;
    return res;
  }
  DeviceGuard g(rounds_.device());
  rounds_.reserve(opt.max_intervals);
  const bool swapped = a > b;
  const double lo = swapped ? b : a, hi = swapped ? a : b;
  const double hw0 = 0.5 * ((hi - lo) / static_cast<double>(opt.panels));
  static_cast<AdaptResult&>(res) = run(
      detail::adapt_job(lo, hi, opt, intervals_out, capacity, swapped), hw0, omega, kind, true);
  if (swapped) res.value = -res.value;
  res.reason = osc_reason(res);
  return res;
}

OscResult ExprAdaptiveOsc::integrate_tail(double a, double omega, OscKind kind,
                                          const AdaptOptions& opt, const OscTailOptions& topt) {
#pragma clang fp contract(off)  // the numpy model repeats these lines
  osc_check(a, std::numeric_limits<double>::infinity(), omega, opt, true, topt);
  OscResult res;
  res.omega = omega;
  res.kind = osc_kind_name(kind);
  res.range = "upper";
  res.tol = opt.atol;
  DeviceGuard g(rounds_.device());
  AdaptOptions o = opt;
  o.unbounded = false;
  o.rtol = 0.0;
  o.panels = topt.panels;
  rounds_.reserve(o.max_intervals);
  const double w = std::fabs(omega);
  const double cycle = ((2.0 * std::floor(w) + 1.0) * 3.141592653589793) / w;
  const double hw0 = 0.5 * (cycle / static_cast<double>(o.panels));
  const double p = 0.9;
  double share = 1.0 - p, psum = 0.0, errsum = 0.0, first_r = 0.0, last_r = 0.0, est = 0.0;
  std::vector<double> sums, results;
  bool all_converged = true, stopped = false;
  for (int k = 1; k <= topt.max_cycles && !stopped; ++k) {
    const double lo = a + static_cast<double>(k - 1) * cycle;
    const double hi = a + static_cast<double>(k) * cycle;
    o.atol = opt.atol * share;
    share = share * p;
    const AdaptResult r = run(detail::adapt_job(lo, hi, o, nullptr, 0), hw0, omega, kind, true);
    res.device_ms += r.device_ms;
    ++res.cycles;
    psum = psum + r.value;
    errsum = errsum + r.err_est;
    res.resabs = res.resabs + r.resabs;
    res.evals += r.evals;
    res.rounds += r.rounds;
    res.intervals += r.intervals;
    res.splits += r.splits;
    res.floor += r.floor;
    res.forced += r.forced;
    res.nonfinite += r.nonfinite;
    res.capped = res.capped || r.capped;
    all_converged = all_converged && r.converged;
    if (k == 1) first_r = r.resabs;
    last_r = r.resabs;
    sums.push_back(psum);
    res.value = psum;
    if (r.nonfinite != 0 || !std::isfinite(psum)) break;
    if (k < 3) continue;
    est = 50.0 * std::fabs(r.value);
    if (errsum + est <= opt.atol) {  // the sum itself: not an earlier cycle's extrapolation
      res.extrapolated = false;
      stopped = true;
      break;
    }
    results.push_back(osc_epsilon(sums.data(), static_cast<int>(sums.size())));
    const size_t m = results.size();
    res.value = results[m - 1];
    res.extrapolated = true;
    if (m < 3) {
      est = std::numeric_limits<double>::infinity();
      continue;
    }
    est = std::fabs(results[m - 1] - results[m - 2]) + std::fabs(results[m - 1] - results[m - 3]);
    if (errsum + est <= opt.atol) stopped = true;
  }
  if (res.cycles < 3) est = std::numeric_limits<double>::infinity();
  res.err_est = errsum + est;
  const bool decays = res.cycles >= 2 && last_r < first_r;
  res.converged = stopped && all_converged && !res.capped && res.nonfinite == 0 && decays;
  if (!res.converged) {
    if (res.nonfinite != 0) res.reason = "f was not finite on " + std::to_string(res.nonfinite) +
                                         " intervals (both ends of every interval are evaluated)";
    else if (res.capped) res.reason = "max_intervals was reached in a cycle";
    else if (!decays) res.reason = "no decay: the last cycle's integral of |f| is not below the "
                                   "first one's, so the Fourier integral does not converge";
    else if (!stopped) res.reason = "max_cycles = " + std::to_string(topt.max_cycles) +
                                    " cycles did not bring the estimate within atol";
    else res.reason = "a cycle did not reach its share of atol";
  }
  return res;
}

double ExprAdaptiveOsc::time(double a, double b, double omega, OscKind kind,
                             const AdaptOptions& opt, int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive timing request");
  osc_check(a, b, omega, opt);
  if (a == b) return 0.0;
  DeviceGuard g(rounds_.device());
  rounds_.reserve(opt.max_intervals);
  const double lo = std::min(a, b), hi = std::max(a, b);
  const double hw0 = 0.5 * ((hi - lo) / static_cast<double>(opt.panels));
  const detail::AdaptJob job = detail::adapt_job(lo, hi, opt, nullptr, 0);
  return rounds_.time(iters, [&] { (void)run(job, hw0, omega, kind, false); });
}

}  // namespace miint
