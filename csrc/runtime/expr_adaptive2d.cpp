// Adaptive double integrals of a runtime f(x, y) over a rectangle to a requested tolerance:
// the tensor product of the Gauss-Kronrod (7, 15) pair on a list of rectangles, bisected by
// rounds along the axis with the larger error (see miint/expr.hpp, ExprAdaptive2D).
#include <algorithm>
#include <cmath>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kBlock = 256;
using detail::hex;
using detail::num;

// "{t0, t1, ...}" of `count` doubles as hex floats.
std::string table(const double* v, int count) {
  std::string s = "{";
  for (int j = 0; j < count; ++j) s += (j ? ", " : "") + hex(v[j]);
  return s + "}";
}
}  // namespace

void adapt2d_check(double ax, double bx, double ay, double by, const Adapt2DOptions& o) {
  const std::string what = "adaptive 2-D: ";
  MIINT_CHECK(std::isfinite(ax) && std::isfinite(bx) && std::isfinite(bx - ax),
              what + "ax = " + num(ax) + " and bx = " + num(bx) +
                  " must be finite, and bx - ax too");
  MIINT_CHECK(std::isfinite(ay) && std::isfinite(by) && std::isfinite(by - ay),
              what + "ay = " + num(ay) + " and by = " + num(by) +
                  " must be finite, and by - ay too");
  MIINT_CHECK(std::isfinite((bx - ax) * (by - ay)),
              what + "the area (bx - ax) * (by - ay) = " + num((bx - ax) * (by - ay)) +
                  " must be finite");
  detail::adapt_check_tolerances(what, o.rtol, o.atol, o.max_intervals);
  MIINT_CHECK(o.panels_x >= 1 && o.panels_y >= 1 && o.panels_x <= o.max_intervals &&
                  o.panels_y <= o.max_intervals / o.panels_x,
              what + "panels_x * panels_y = " + std::to_string(o.panels_x) + " * " +
                  std::to_string(o.panels_y) + " must be 1..max_intervals = " +
                  std::to_string(o.max_intervals) + ", each factor at least 1");
  detail::adapt_check_depth(what, o.max_depth, " (per axis)");
}

namespace detail {

namespace {
// The rule's one table (gk15_nodes and its weights): the non-negative nodes from the centre
// outwards, their Kronrod weights, and the Gauss weights of nodes 0, 2, 4, 6.
struct Gk15Table {
  double t[8], wk[8], wg[4];
  Gk15Table() {
    const std::vector<double> t15 = gk15_nodes(), wk15 = gk15_weights(), wg7 = gk7_weights();
    for (int j = 0; j < 8; ++j) {
      t[j] = t15[7 + j];
      wk[j] = wk15[7 + j];
    }
    for (int j = 0; j < 4; ++j) wg[j] = wg7[3 + j];
  }
};
}  // namespace

std::string adapt2d_table_source() {
  const Gk15Table g;
  return R"(
// The y direction's table, read with a wave-uniform index: scalar loads.
__constant__ double miint_gk_t[8] = )" + table(g.t, 8) + R"(;
__constant__ double miint_gk_wk[8] = )" + table(g.wk, 8) + R"(;
__constant__ double miint_gk_wg[4] = )" + table(g.wg, 4) + R"(;
)";
}

// A row's fifteen evaluations, printed: the centre, then a pair of nodes per line. With
// `columns` a pair's macro also takes the numbers of its two columns, 2 j - 1 and 2 j.
std::string adapt2d_row_source(bool columns) {
  const Gk15Table g;
  std::string row = "    MIINT_ROW_CENTRE(" + hex(g.wk[0]) + ", " + hex(g.wg[0]) + ")\n";
  for (int j = 1; j < 8; ++j) {
    const std::string cols =
        columns ? ", " + std::to_string(2 * j - 1) + ", " + std::to_string(2 * j) : "";
    if (j % 2 == 0)
      row += "    MIINT_ROW_GAUSS_PAIR(" + hex(g.t[j]) + ", " + hex(g.wk[j]) + ", " +
             hex(g.wg[j / 2]) + cols + ")\n";
    else
      row += "    MIINT_ROW_PAIR(" + hex(g.t[j]) + ", " + hex(g.wk[j]) + cols + ")\n";
  }
  return row;
}

}  // namespace detail

std::string expr_adapt2d_source(const std::string& expr) {
  detail::expr_check_named(expr);
  return std::string(detail::kRtcPrelude) + R"(
__device__ __forceinline__ double miint_f(double x, double y) {
  (void)x; (void)y;
  return ()" + expr + R"();
}
)" + detail::adapt2d_table_source() + R"(
// One row of the (7, 15) x (7, 15) product at a fixed y: f at the centre cx and at the seven
// pairs fma(hx, -+t, cx), from the centre outwards, the three row sums carried by fma.
#define MIINT_ROW_CENTRE(wk, wg) \
  { const double f0 = miint_f(cx, y); rk = wk * f0; rg = wg * f0; ra = wk * fabs(f0); }
#define MIINT_ROW_PAIR(t, wk)                                                          \
  { const double f1 = miint_f(fma(hx, -t, cx), y), f2 = miint_f(fma(hx, t, cx), y);     \
    rk = fma(wk, f1 + f2, rk); ra = fma(wk, fabs(f1) + fabs(f2), ra); }
#define MIINT_ROW_GAUSS_PAIR(t, wk, wg)                                                \
  { const double f1 = miint_f(fma(hx, -t, cx), y), f2 = miint_f(fma(hx, t, cx), y);     \
    rk = fma(wk, f1 + f2, rk); ra = fma(wk, fabs(f1) + fabs(f2), ra);                  \
    rg = fma(wg, f1 + f2, rg); }

// The product rule on [x0, x1] x [y0, y1]. The rows run in the 1-D order too: row 0 is the
// centre cy, rows 2 j - 1 and 2 j are fma(hy, -+t_j, cy); a pair's row sums are added, then
// carried by fma onto KK, GK, RA (Kronrod weight) and, for the even j, onto GG and KG (Gauss
// weight). The loop over the rows stays rolled: its body is one row's fifteen evaluations, and
// whatever f does with x alone is formed once in front of it.
__device__ __forceinline__ void miint_gk15x15(double2 xr, double2 yr, double* k, double* err,
                                              double* ex, double* ey, double* r) {
#pragma clang fp contract(off)  // K, G and the direction errors are rounded before they are compared
  const double hx = 0.5 * (xr.y - xr.x), cx = xr.x + hx;
  const double hy = 0.5 * (yr.y - yr.x), cy = yr.x + hy;
  double kk = 0.0, gg = 0.0, gk = 0.0, kg = 0.0, aa = 0.0;
  double pk = 0.0, pg = 0.0, pa = 0.0;  // the row at -t_j, kept for its partner
#pragma unroll 1
  for (int row = 0; row < 15; ++row) {
    const int j = (row + 1) >> 1;
    const double t = miint_gk_t[j];
    const double y = row == 0 ? cy : fma(hy, (row & 1) ? -t : t, cy);
    double rk, rg, ra;
)" + detail::adapt2d_row_source(false) + detail::kAdapt2DCombine +
         detail::adapt_round_source(2, detail::adapt2d_eval_source(
             "// One rectangle per lane: the same 225 evaluations in every lane, 16-byte extent "
             "loads.\n",
             "miint_adapt2d_eval", "miint_gk15x15"));
}

namespace detail {

// The end of a row of the rule's loop and of the rule: the row's three sums onto the five of
// the rectangle, then K, err, ex, ey and R. Shared by miint_gk15x15 and its region twin.
const char* const kAdapt2DCombine = R"(    if (row == 0) {
      const double wk = miint_gk_wk[0], wg = miint_gk_wg[0];
      kk = wk * rk; gk = wk * rg; aa = wk * ra;
      gg = wg * rg; kg = wg * rk;
    } else if (row & 1) {
      pk = rk; pg = rg; pa = ra;
    } else {
      const double wk = miint_gk_wk[j];
      const double tk = pk + rk, tg = pg + rg, ta = pa + ra;
      kk = fma(wk, tk, kk); gk = fma(wk, tg, gk); aa = fma(wk, ta, aa);
      if ((j & 1) == 0) {
        const double wg = miint_gk_wg[j >> 1];
        gg = fma(wg, tg, gg); kg = fma(wg, tk, kg);
      }
    }
  }
  const double s = hx * hy;
  const double kv = s * kk;
  *k = kv;
  *err = fabs(kv - s * gg);
  *ex = fabs(kv - s * gk);
  *ey = fabs(kv - s * kg);
  *r = s * aa;
}
)";

std::string adapt2d_eval_source(const std::string& comment, const std::string& name,
                                const std::string& rule) {
  return adapt_eval_source(
      comment, name,
      R"(unsigned long long n, const double2* __restrict__ xs, const double2* __restrict__ ys,
    double* __restrict__ k, double* __restrict__ err, double2* __restrict__ dir,
    double* __restrict__ r, double* __restrict__ part_k)",
      "    double e, ex, ey, a;\n    " + rule + "(xs[i], ys[i], &v, &e, &ex, &ey, &a);\n",
      "    dir[i] = make_double2(ex, ey);\n");
}

namespace {
// The job of a checked call (each axis ascending) and the launch of the rounds' own evaluation
// kernel, which takes miint_adapt2d_eval's arguments.
AdaptJob job2d(double ax, double bx, double ay, double by, const Adapt2DOptions& opt, double* out,
               uint64_t capacity) {
  return {std::min(ax, bx), std::max(ax, bx), std::min(ay, by), std::max(ay, by), opt.panels_x,
          opt.panels_y, opt.rtol, opt.atol, opt.max_intervals, opt.max_depth, out, capacity,
          false};
}

AdaptRounds::Eval eval2d(AdaptRounds& rounds) {
  return [&rounds](const AdaptItems& it) {
    rounds.module().launch(AdaptRounds::kEval, it.blocks, 1, kBlock, it.stream, it.n, it.xs,
                           it.ys, it.k, it.err, it.dir, it.r, it.part_k);
  };
}
}  // namespace

Adapt2DResult adapt2d_integrate(AdaptRounds& rounds, double ax, double bx, double ay, double by,
                                const Adapt2DOptions& opt, double* rects_out, uint64_t capacity) {
  adapt2d_check(ax, bx, ay, by, opt);
  rounds.check_capacity(rects_out, capacity, opt.max_intervals);
  if (ax == bx || ay == by) {
    Adapt2DResult r;
    r.tol = opt.atol;
    r.converged = true;
    return r;
  }
  DeviceGuard g(rounds.device());
  rounds.reserve(opt.max_intervals);
  Adapt2DResult r = rounds.integrate<Adapt2DResult>(
      job2d(ax, bx, ay, by, opt, rects_out, capacity), 225, eval2d(rounds));
  if ((ax > bx) != (ay > by)) r.value = -r.value;
  return r;
}

double adapt2d_time(AdaptRounds& rounds, double ax, double bx, double ay, double by,
                    const Adapt2DOptions& opt, int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive 2-D timing request");
  adapt2d_check(ax, bx, ay, by, opt);
  if (ax == bx || ay == by) return 0.0;
  DeviceGuard g(rounds.device());
  rounds.reserve(opt.max_intervals);
  const AdaptJob j = job2d(ax, bx, ay, by, opt, nullptr, 0);
  const AdaptRounds::Eval e = eval2d(rounds);
  return rounds.time(iters, [&] { (void)rounds.run<Adapt2DResult>(j, 225, e); });
}

}  // namespace detail

std::string expr_adapt2d_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_adapt2d_source(expr), expr);
}

ExprAdaptive2D::ExprAdaptive2D(const std::string& expr, int device)
    : expr_(expr), rounds_(2, expr_adapt2d_compile(expr), "miint_adapt2d_eval", device) {}

Adapt2DResult ExprAdaptive2D::integrate(double ax, double bx, double ay, double by,
                                        const Adapt2DOptions& opt, double* rects_out,
                                        uint64_t capacity) {
  return detail::adapt2d_integrate(rounds_, ax, bx, ay, by, opt, rects_out, capacity);
}

double ExprAdaptive2D::time(double ax, double bx, double ay, double by, const Adapt2DOptions& opt,
                            int iters) {
  return detail::adapt2d_time(rounds_, ax, bx, ay, by, opt, iters);
}

}  // namespace miint
