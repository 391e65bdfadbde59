// Adaptive double integrals of a runtime f(x, y) between two curves, y from ylo(x) to yhi(x):
// the region mapped onto [ax, bx] x [0, 1] and the rounds of rectangles (detail::AdaptRounds) on
// the mapped integrand, around its own evaluation kernel (see miint/expr.hpp, ExprAdaptiveRegion).
#include <cctype>
#include <cstdio>
#include <vector>

#include "miint/expr.hpp"

namespace miint {

namespace {
// expr_check names the character or word it refuses; here also which of the three it is.
void check_one(const std::string& which, const std::string& expr) {
  try {
    expr_check(expr);
  } catch (const std::exception& e) {
    fail(which + " '" + expr + "' is rejected: " + e.what(), __FILE__, __LINE__);
  }
}

bool ident_char(char c) { return std::isalnum(static_cast<unsigned char>(c)) || c == '_'; }

// A limit is a function of x alone: the identifier y in it is refused, naming the limit.
void check_limit(const std::string& which, const std::string& expr) {
  check_one(which, expr);
  for (size_t i = 0; i < expr.size(); ++i) {
    if (expr[i] != 'y') continue;
    const bool starts = i == 0 || !(ident_char(expr[i - 1]) || expr[i - 1] == '.');
    const bool ends = i + 1 == expr.size() || !ident_char(expr[i + 1]);
    MIINT_CHECK(!(starts && ends), which + " '" + expr + "' is rejected: a limit in y is a "
                                       "function of x alone and may not mention y");
  }
}
}  // namespace

std::string expr_region_source(const std::string& expr, const std::string& ylo,
                               const std::string& yhi) {
  check_one("the integrand", expr);
  check_limit("the lower limit y_lo", ylo);
  check_limit("the upper limit y_hi", yhi);
  return std::string(detail::kRtcPrelude) + R"(
__device__ __forceinline__ double miint_f(double x, double y) {
  (void)x; (void)y;
  return ()" + expr + R"();
}
__device__ __forceinline__ double miint_ylo(double x) {
  (void)x;
  return ()" + ylo + R"();
}
__device__ __forceinline__ double miint_yhi(double x) {
  (void)x;
  return ()" + yhi + R"();
}
)" + detail::adapt2d_table_source() + R"(
// Column i of the product: the lower limit g and the signed height w = yhi - g at x node i
// (0 the centre cx, 2 j - 1 and 2 j at fma(hx, -+t_j, cx)). Formed once per rectangle.
#define MIINT_LIMITS(i, xi) \
  const double g##i = miint_ylo(xi); const double w##i = miint_yhi(xi) - g##i;
#define MIINT_LIMITS_CENTRE() MIINT_LIMITS(0, cx)
#define MIINT_LIMITS_PAIR(t, a, b) \
  MIINT_LIMITS(a, fma(hx, -t, cx)) MIINT_LIMITS(b, fma(hx, t, cx))

// One row of the product at a fixed v: the mapped integrand f(x_i, fma(w_i, v, g_i)) * w_i at
// the centre and at the seven pairs of columns a (at -t) and b (at +t), from the centre
// outwards, the three row sums carried by fma as in miint_gk15x15.
#define MIINT_MAPPED(xi, i) (miint_f(xi, fma(w##i, v, g##i)) * w##i)
#define MIINT_ROW_CENTRE(wk, wg) \
  { const double f0 = MIINT_MAPPED(cx, 0); rk = wk * f0; rg = wg * f0; ra = wk * fabs(f0); }
#define MIINT_ROW_PAIR(t, wk, a, b)                                                    \
  { const double f1 = MIINT_MAPPED(fma(hx, -t, cx), a), f2 = MIINT_MAPPED(fma(hx, t, cx), b); \
    rk = fma(wk, f1 + f2, rk); ra = fma(wk, fabs(f1) + fabs(f2), ra); }
#define MIINT_ROW_GAUSS_PAIR(t, wk, wg, a, b)                                          \
  { const double f1 = MIINT_MAPPED(fma(hx, -t, cx), a), f2 = MIINT_MAPPED(fma(hx, t, cx), b); \
    rk = fma(wk, f1 + f2, rk); ra = fma(wk, fabs(f1) + fabs(f2), ra);                  \
    rg = fma(wg, f1 + f2, rg); }

// The product rule on [x0, x1] x [v0, v1] of the mapped integrand. The fifteen columns' limits
// are formed explicitly in front of the loop and stay in registers: a limit costs 30 calls a
// rectangle, not 450. The rows run as in miint_gk15x15, the loop over them rolled, and the
// rule ends in the same text.
__device__ __forceinline__ void miint_region_gk15x15(double2 xr, double2 yr, double* k,
                                                     double* err, double* ex, double* ey,
                                                     double* r) {
#pragma clang fp contract(off)  // w = yhi - g and f * w are rounded on their own, as K and G are
  const double hx = 0.5 * (xr.y - xr.x), cx = xr.x + hx;
  const double hy = 0.5 * (yr.y - yr.x), cy = yr.x + hy;
)" + [] {
    // the columns' limits, printed: the centre, then a pair of columns per line
    const std::vector<double> t15 = gk15_nodes();
    std::string s = "  MIINT_LIMITS_CENTRE()\n";
    for (int j = 1; j < 8; ++j) {
      char b[96];
      std::snprintf(b, sizeof b, "  MIINT_LIMITS_PAIR(%a, %d, %d)\n", t15[7 + j], 2 * j - 1, 2 * j);
      s += b;
    }
    return s;
  }() + R"(  double kk = 0.0, gg = 0.0, gk = 0.0, kg = 0.0, aa = 0.0;
  double pk = 0.0, pg = 0.0, pa = 0.0;  // the row at -t_j, kept for its partner
#pragma unroll 1
  for (int row = 0; row < 15; ++row) {
    const int j = (row + 1) >> 1;
    const double t = miint_gk_t[j];
    const double v = row == 0 ? cy : fma(hy, (row & 1) ? -t : t, cy);
    double rk, rg, ra;
)" + detail::adapt2d_row_source(true) + detail::kAdapt2DCombine +
         detail::adapt_round_source(2, detail::adapt2d_eval_source(
             "// One rectangle of (x, v) per lane: 30 limit evaluations, then the same 225 "
             "evaluations of the\n// mapped integrand in every lane. The arguments are "
             "miint_adapt2d_eval's.\n",
             "miint_region_eval", "miint_region_gk15x15"));
}

std::string expr_region_compile(const std::string& expr, const std::string& ylo,
                                const std::string& yhi) {
  return detail::rtc_compile_cached(expr_region_source(expr, ylo, yhi),
                                    expr + "' between '" + ylo + "' and '" + yhi);
}

ExprAdaptiveRegion::ExprAdaptiveRegion(const std::string& expr, const std::string& ylo,
                                       const std::string& yhi, int device)
    : expr_(expr), ylo_(ylo), yhi_(yhi),
      rounds_(2, expr_region_compile(expr, ylo, yhi), "miint_region_eval", device) {}

Adapt2DResult ExprAdaptiveRegion::integrate(double ax, double bx, const Adapt2DOptions& opt,
                                            double* rects_out, uint64_t capacity) {
  return detail::adapt2d_integrate(rounds_, ax, bx, 0.0, 1.0, opt, rects_out, capacity);
}

double ExprAdaptiveRegion::time(double ax, double bx, const Adapt2DOptions& opt, int iters) {
  return detail::adapt2d_time(rounds_, ax, bx, 0.0, 1.0, opt, iters);
}

}  // namespace miint
