// Adaptive Gauss-Kronrod (7, 15) integration of a runtime integrand to a requested tolerance
// (see miint/expr.hpp, ExprAdaptive).
#include <algorithm>
#include <cmath>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kAdaptBlock = 256;

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

using detail::hex;
using detail::num;
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
  detail::adapt_check_tolerances(what, o.rtol, o.atol, o.max_intervals);
  MIINT_CHECK(o.panels >= 1 && o.panels <= o.max_intervals,
              what + "panels = " + std::to_string(o.panels) + " must be 1..max_intervals = " +
                  std::to_string(o.max_intervals));
  detail::adapt_check_depth(what, o.max_depth);
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

AdaptJob adapt_job(double lo, double hi, const AdaptOptions& opt, double* out, uint64_t capacity,
                   bool descending) {
  return {lo, hi, 0.0, 0.0, opt.panels, 1, opt.rtol, opt.atol, opt.max_intervals, opt.max_depth,
          out, capacity, descending};
}
}  // namespace detail

std::string expr_adapt_unbounded_source(const std::string& expr) {
  detail::expr_check_named(expr);
  std::string src = std::string(detail::kRtcPrelude) + detail::adapt_unbounded_rule_source(expr, "", "");
  // miint_adapt_eval's twins: the interval is one of t in [0, 1], the block sums and partials
  // are the same.
  const char* names[3] = {"upper", "lower", "both"};
  for (int kind = 1; kind <= 3; ++kind)
    src += "\n" + detail::adapt_eval_source(
        "", std::string("miint_adapt_eval_") + names[kind - 1],
        R"(unsigned long long n, const double2* __restrict__ list, double end, double* __restrict__ k,
    double* __restrict__ err, double* __restrict__ r, double* __restrict__ part_k)",
        "    const double2 iv = list[i];\n    double e, a;\n    miint_gk15(iv.x, iv.y, " +
            std::to_string(kind) + ", end, &v, &e, &a);\n");
  return src;
}

std::string expr_adapt_unbounded_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_adapt_unbounded_source(expr), expr);
}

std::string expr_adapt_source(const std::string& expr) {
  detail::expr_check_named(expr);
  return std::string(detail::kRtcPrelude) + detail::adapt_rule_source(expr, "", "") +
         detail::adapt_round_source(1, detail::adapt_eval_source(
             "// One interval per lane: the same fifteen evaluations in every lane, 16-byte "
             "endpoint loads.\n",
             "miint_adapt_eval",
             R"(unsigned long long n, const double2* __restrict__ list, double* __restrict__ k,
    double* __restrict__ err, double* __restrict__ r, double* __restrict__ part_k)",
             "    const double2 iv = list[i];\n    double e, a;\n"
             "    miint_gk15(iv.x, iv.y, &v, &e, &a);\n"));
}

std::string expr_adapt_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_adapt_source(expr), expr);
}

ExprAdaptive::ExprAdaptive(const std::string& expr, int device)
    : expr_(expr), rounds_(1, expr_adapt_compile(expr), "miint_adapt_eval", device) {}

// The evaluation launch of a call's range: miint_adapt_eval, or the twin of the kind (kernels 0,
// 1, 2 of unbounded_, compiled, cached per expression, and loaded at the object's first
// unbounded call) with the finite end.
detail::AdaptRounds::Eval ExprAdaptive::eval(double a, double b) {
  const AdaptRange kind = adapt_range(a, b);
  if (kind == AdaptRange::kFinite)
    return [this](const detail::AdaptItems& it) {
      rounds_.module().launch(detail::AdaptRounds::kEval, it.blocks, 1, kAdaptBlock, it.stream,
                              it.n, it.xs, it.k, it.err, it.r, it.part_k);
    };
  if (!unbounded_)
    unbounded_.reset(new detail::RtcModule(
        expr_adapt_unbounded_compile(expr_), rounds_.device(), rounds_.stream(),
        {"miint_adapt_eval_upper", "miint_adapt_eval_lower", "miint_adapt_eval_both"}));
  const double end = std::isinf(a) ? b : a;  // the finite end of a half-infinite range
  return [this, kind, end](const detail::AdaptItems& it) {
    unbounded_->launch(static_cast<size_t>(kind) - 1, it.blocks, 1, kAdaptBlock, it.stream, it.n,
                       it.xs, end, it.k, it.err, it.r, it.part_k);
  };
}

// f on [min(a, b), max(a, b)], or g on [0, 1] in t: a mapped range stays ascending in t.
detail::AdaptJob ExprAdaptive::job(double a, double b, const AdaptOptions& opt, double* out,
                                   uint64_t capacity) {
  if (adapt_range(a, b) != AdaptRange::kFinite)
    return detail::adapt_job(0.0, 1.0, opt, out, capacity);
  return detail::adapt_job(std::min(a, b), std::max(a, b), opt, out, capacity, a > b);
}

AdaptResult ExprAdaptive::integrate(double a, double b, const AdaptOptions& opt,
                                    double* intervals_out, uint64_t capacity) {
  adapt_check(a, b, opt);
  rounds_.check_capacity(intervals_out, capacity, opt.max_intervals);
  if (a == b) {
    AdaptResult r;
    r.tol = opt.atol;
    r.converged = true;
    return r;
  }
  DeviceGuard g(rounds_.device());
  rounds_.reserve(opt.max_intervals);
  AdaptResult r = rounds_.integrate<AdaptResult>(job(a, b, opt, intervals_out, capacity), 15,
                                                 eval(a, b));
  r.range = adapt_range_name(adapt_range(a, b));
  if (a > b) r.value = -r.value;
  return r;
}

double ExprAdaptive::time(double a, double b, const AdaptOptions& opt, int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive timing request");
  adapt_check(a, b, opt);
  if (a == b) return 0.0;
  DeviceGuard g(rounds_.device());
  rounds_.reserve(opt.max_intervals);
  const detail::AdaptJob j = job(a, b, opt, nullptr, 0);
  const detail::AdaptRounds::Eval e = eval(a, b);
  return rounds_.time(iters, [&] { (void)rounds_.run<AdaptResult>(j, 15, e); });
}

}  // namespace miint
