// Adaptive double integrals of a runtime f(x, y) over a rectangle to a requested tolerance:
// the tensor product of the Gauss-Kronrod (7, 15) pair on a list of rectangles, bisected by
// rounds along the axis with the larger error (see miint/expr.hpp, ExprAdaptive2D).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "miint/expr.hpp"

namespace miint {

namespace {
constexpr int kBlock = 256;
enum { kInit, kEval, kClose, kDecide, kPrefix, kScatter };  // module_'s kernels

// The device's totals: words 0..7 are doubles, 8..17 counters. miint_adapt2d_prefix stores the
// same eighteen words into the pinned record at the end of every round.
enum { kS, kE, kR, kTol, kSumK };
enum { kAccepted = 8, kSplits, kFloor, kForced, kNonfinite, kNext, kCapped, kBase, kSplitsX,
       kSplitsY };
constexpr size_t kStateWords = 18;

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
  MIINT_CHECK(o.rtol >= 0.0 && o.atol >= 0.0 && std::isfinite(o.rtol) && std::isfinite(o.atol) &&
                  (o.rtol > 0.0 || o.atol > 0.0),
              what + "rtol = " + num(o.rtol) + " and atol = " + num(o.atol) +
                  " must be finite and >= 0, and not both 0");
  MIINT_CHECK(o.max_intervals >= 1 && o.max_intervals <= kAdaptMaxIntervalsLimit,
              what + "max_intervals = " + std::to_string(o.max_intervals) + " must be 1..2^26");
  MIINT_CHECK(o.panels_x >= 1 && o.panels_y >= 1 && o.panels_x <= o.max_intervals &&
                  o.panels_y <= o.max_intervals / o.panels_x,
              what + "panels_x * panels_y = " + std::to_string(o.panels_x) + " * " +
                  std::to_string(o.panels_y) + " must be 1..max_intervals = " +
                  std::to_string(o.max_intervals) + ", each factor at least 1");
  MIINT_CHECK(o.max_depth >= 0 && o.max_depth <= kAdaptMaxDepthLimit,
              what + "max_depth = " + std::to_string(o.max_depth) + " must be 0..200 (per axis)");
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
)" + detail::adapt2d_row_source(false) + detail::kAdapt2DCombine + detail::kAdapt2DInit + R"(
// One rectangle per lane: the same 225 evaluations in every lane, 16-byte extent loads.
extern "C" __global__ __launch_bounds__(256) void miint_adapt2d_eval(
    unsigned long long n, const double2* __restrict__ xs, const double2* __restrict__ ys,
    double* __restrict__ k, double* __restrict__ err, double2* __restrict__ dir,
    double* __restrict__ r, double* __restrict__ part_k) {
  __shared__ double red[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  double v = 0.0;
  if (i < n) {
    double e, ex, ey, a;
    miint_gk15x15(xs[i], ys[i], &v, &e, &ex, &ey, &a);
    k[i] = v;
    err[i] = e;
    dir[i] = make_double2(ex, ey);
    r[i] = a;
  }
  MIINT_BLOCK_SUM(v, red);
  if (threadIdx.x == 0) part_k[blockIdx.x] = MIINT_RED(red);
}
)" + detail::kAdapt2DRound;
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

// The kernels of a round that do not evaluate f: miint_adapt2d_init in front of the evaluation
// kernel, the other four behind it. ExprAdaptiveRegion's source carries the same text.
const char* const kAdapt2DInit = R"(
// st[0..7] as doubles: S_acc, E_acc, R_acc, tol, sum_K; st[8..17]: accepted, splits, floor,
// forced, nonfinite, next, capped, base (the rectangles accepted before this round), splits_x,
// splits_y.
#define MIINT_ST_D(st, i) (((double*)(st))[i])

// The first list: rectangle i = iy * px + ix (x fastest) of px x py equal ones; per axis the
// edges a + ((b - a) k) / panels, the last one b, as miint_adapt_init forms them.
extern "C" __global__ __launch_bounds__(256) void miint_adapt2d_init(
    double ax, double bx, double ay, double by, unsigned long long px, unsigned long long py,
    double2* __restrict__ xs, double2* __restrict__ ys, unsigned* __restrict__ depth) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= px * py) return;
  const unsigned long long ix = i % px, iy = i / px;
  const double wx = bx - ax, wy = by - ay, fx = (double)px, fy = (double)py;
  const double x0 = ax + (wx * (double)ix) / fx;
  const double x1 = ix + 1 == px ? bx : ax + (wx * (double)(ix + 1)) / fx;
  const double y0 = ay + (wy * (double)iy) / fy;
  const double y1 = iy + 1 == py ? by : ay + (wy * (double)(iy + 1)) / fy;
  xs[i] = make_double2(x0, x1);
  ys[i] = make_double2(y0, y1);
  depth[i] = 0u;
}
)";

const char* const kAdapt2DRound = R"(
// sum_K over the nb workgroups' partials, then the round's tolerance. A NaN sum gives a NaN
// tolerance (atol > NaN is false).
extern "C" __global__ __launch_bounds__(256) void miint_adapt2d_close(
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

// Per rectangle the axis and the decision (miint/expr.hpp has the order); per workgroup the
// number to split (and of those along x), the three counters and five sums: the accepted K,
// err and R, the K and err to be split. depth holds the x depth in its low half, the y depth
// in its high half. split: 0 accepted, 1 bisect x, 2 bisect y.
extern "C" __global__ __launch_bounds__(256) void miint_adapt2d_decide(
    unsigned long long n, const double2* __restrict__ xs, const double2* __restrict__ ys,
    const double* __restrict__ k, const double* __restrict__ err,
    const double2* __restrict__ dir, const double* __restrict__ r,
    const unsigned* __restrict__ depth, double box_x, double box_y, unsigned max_depth,
    const unsigned long long* __restrict__ st, unsigned char* __restrict__ split,
    unsigned* __restrict__ blk_counts, double* __restrict__ blk_sums) {
  __shared__ double red[5][4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const double tol = ((const double*)st)[3];
  double ak = 0.0, ae = 0.0, ar = 0.0, pk = 0.0, pe = 0.0;
  int how = 0;  // 1 nonfinite, 2 within tolerance, 3 floor, 4 forced, 5 split
  bool along_x = false;
  if (i < n) {
    const double2 xr = xs[i], yr = ys[i], d = dir[i];
    const double kv = k[i], ev = err[i], rv = r[i];
    const double wx = xr.y - xr.x, wy = yr.y - yr.x;
    along_x = d.x > d.y ? true : d.y > d.x ? false : wx * box_y >= wy * box_x;
    const double lo = along_x ? xr.x : yr.x, hi = along_x ? xr.y : yr.y;
    const double c = lo + 0.5 * (hi - lo);
    const unsigned dep = along_x ? depth[i] & 0xffffu : depth[i] >> 16;
    if (!(isfinite(kv) && isfinite(ev))) how = 1;
    else if (!(ev > (tol * (wx * wy)) / (box_x * box_y))) how = 2;
    else if (ev <= 0x1.9p-47 * rv) how = 3;  // 50 * 2^-52
    else if (dep >= max_depth || c == lo || c == hi) how = 4;
    else how = 5;
    split[i] = how == 5 ? (along_x ? 1 : 2) : 0;
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
  const int n_split_x = __syncthreads_count(how == 5 && along_x);
  MIINT_BLOCK_SUM(ak, red[0]);
  MIINT_BLOCK_SUM(ae, red[1]);
  MIINT_BLOCK_SUM(ar, red[2]);
  MIINT_BLOCK_SUM(pk, red[3]);
  MIINT_BLOCK_SUM(pe, red[4]);
  if (threadIdx.x == 0) {
    unsigned* bc = blk_counts + 5ull * blockIdx.x;
    bc[0] = (unsigned)n_split;
    bc[1] = (unsigned)n_floor;
    bc[2] = (unsigned)n_forced;
    bc[3] = (unsigned)n_nonfinite;
    bc[4] = (unsigned)n_split_x;
    double* bs = blk_sums + 5ull * blockIdx.x;
    for (int q = 0; q < 5; ++q) bs[q] = MIINT_RED(red[q]);
  }
}

// One workgroup over the nb workgroups of the round. Thread t owns the contiguous run of
// per = ceil(nb / 256) of them from t * per: their sums in order, then the block reduction;
// thread 0 scans the 256 runs' split counts, and every thread writes its run's exclusive
// prefixes. Thread 0 then closes the round: capped or not, the totals, the record.
extern "C" __global__ __launch_bounds__(256) void miint_adapt2d_prefix(
    int nb, unsigned long long n, unsigned long long max_intervals,
    const unsigned* __restrict__ blk_counts, const double* __restrict__ blk_sums,
    unsigned* __restrict__ blk_off, unsigned long long* __restrict__ st,
    unsigned long long* __restrict__ record) {
  __shared__ double red[5][4];
  __shared__ unsigned long long runs[256];
  __shared__ unsigned long long cnt[4][4];
  const int per = (nb + 255) / 256;
  const int first = (int)threadIdx.x * per;
  const int last = first + per < nb ? first + per : nb;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned long long n_split = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
  for (int b = first; b < last; ++b) {
    for (int q = 0; q < 5; ++q) s[q] += blk_sums[5ull * b + q];
    n_split += blk_counts[5ull * b];
    c1 += blk_counts[5ull * b + 1];
    c2 += blk_counts[5ull * b + 2];
    c3 += blk_counts[5ull * b + 3];
    c4 += blk_counts[5ull * b + 4];
  }
  runs[threadIdx.x] = n_split;
  for (int o = 32; o > 0; o >>= 1) {
    c1 += __shfl_xor(c1, o, 64);
    c2 += __shfl_xor(c2, o, 64);
    c3 += __shfl_xor(c3, o, 64);
    c4 += __shfl_xor(c4, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    cnt[0][threadIdx.x >> 6] = c1;
    cnt[1][threadIdx.x >> 6] = c2;
    cnt[2][threadIdx.x >> 6] = c3;
    cnt[3][threadIdx.x >> 6] = c4;
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
    const unsigned long long split_x = (cnt[3][0] + cnt[3][1]) + (cnt[3][2] + cnt[3][3]);
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
    st[16] += capped ? 0ull : split_x;
    st[17] += capped ? 0ull : total_split - split_x;
    st[13] = capped ? 0ull : 2ull * total_split;
    st[14] = capped ? 1ull : 0ull;
    for (int q = 0; q < 8; ++q) MIINT_ST_D(record, q) = MIINT_ST_D(st, q);
    for (int q = 8; q < 18; ++q) record[q] = st[q];
  }
  __syncthreads();
  unsigned long long off = runs[threadIdx.x];
  for (int b = first; b < last; ++b) {
    blk_off[b] = (unsigned)off;
    off += blk_counts[5ull * b];
  }
}

// The two children of a rectangle bisected along its axis, that axis's depth + 1, to slots
// 2 p, 2 p + 1 of the next lists, p the number of rectangles split before this one: blk_off
// plus the lanes before it in the workgroup (ballot and popcount per wave, the waves' counts
// through LDS). An accepted rectangle (all of them in a capped round) goes to slot base + (the
// accepted before it) of `done`, if given, as (x0, x1), (y0, y1). Nothing is stored at or past
// next_cap or done_cap.
extern "C" __global__ __launch_bounds__(256) void miint_adapt2d_scatter(
    unsigned long long n, const double2* __restrict__ xs, const double2* __restrict__ ys,
    const unsigned* __restrict__ depth, const unsigned char* __restrict__ split,
    const unsigned* __restrict__ blk_off, const unsigned long long* __restrict__ st,
    double2* __restrict__ next_xs, double2* __restrict__ next_ys,
    unsigned* __restrict__ next_depth, unsigned long long next_cap, double2* __restrict__ done,
    unsigned long long done_cap) {
  __shared__ unsigned waves[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool capped = st[14] != 0ull;
  const bool valid = i < n;
  const unsigned char axis = valid && !capped ? split[i] : (unsigned char)0;
  const bool sp = axis != 0;
  const unsigned long long mask = __ballot(sp);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) waves[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  unsigned before = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  for (unsigned w = 0; w < wave; ++w) before += waves[w];
  if (!valid) return;
  const double2 xr = xs[i], yr = ys[i];
  const unsigned long long p = capped ? 0ull : (unsigned long long)blk_off[blockIdx.x] + before;
  if (sp) {
    if (2ull * p + 1ull < next_cap) {
      if (axis == 1) {
        const double c = xr.x + 0.5 * (xr.y - xr.x);
        const unsigned d = depth[i] + 1u;
        next_xs[2ull * p] = make_double2(xr.x, c);
        next_xs[2ull * p + 1ull] = make_double2(c, xr.y);
        next_ys[2ull * p] = yr;
        next_ys[2ull * p + 1ull] = yr;
        next_depth[2ull * p] = d;
        next_depth[2ull * p + 1ull] = d;
      } else {
        const double c = yr.x + 0.5 * (yr.y - yr.x);
        const unsigned d = depth[i] + 0x10000u;
        next_xs[2ull * p] = xr;
        next_xs[2ull * p + 1ull] = xr;
        next_ys[2ull * p] = make_double2(yr.x, c);
        next_ys[2ull * p + 1ull] = make_double2(c, yr.y);
        next_depth[2ull * p] = d;
        next_depth[2ull * p + 1ull] = d;
      }
    }
  } else if (done != nullptr) {
    const unsigned long long q = st[15] + (i - p);
    if (q < done_cap) {
      done[2ull * q] = xr;
      done[2ull * q + 1ull] = yr;
    }
  }
}
)";

}  // namespace detail

std::string expr_adapt2d_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_adapt2d_source(expr), expr);
}

ExprAdaptive2D::ExprAdaptive2D(const std::string& expr, int device)
    : ExprAdaptive2D(expr, expr_adapt2d_compile(expr), "miint_adapt2d_eval", device) {}

// `code` holds the five kernels every round shares and the evaluation kernel `eval`, which
// takes miint_adapt2d_eval's arguments.
ExprAdaptive2D::ExprAdaptive2D(const std::string& expr, const std::string& code, const char* eval,
                               int device)
    : expr_(expr), device_(device), stream_((set_device(device), Stream())),
      module_(code, device, stream_,
              {"miint_adapt2d_init", eval, "miint_adapt2d_close", "miint_adapt2d_decide",
               "miint_adapt2d_prefix", "miint_adapt2d_scatter"}) {
  DeviceGuard g(device);
  state_ = DeviceBuffer<unsigned long long>(kStateWords);
  record_ = PinnedBuffer<unsigned long long>(kStateWords);
}

// Every buffer holds max_intervals rectangles (or their workgroups): sized once for the
// largest max_intervals asked so far and kept across calls.
void ExprAdaptive2D::reserve(uint64_t m) {
  if (m <= reserved_) return;
  stream_.sync();
  const uint64_t nb = (m + kBlock - 1) / kBlock;
  for (int q = 0; q < 2; ++q) {
    xs_[q] = DeviceBuffer<double>(2 * m);
    ys_[q] = DeviceBuffer<double>(2 * m);
    depth_[q] = DeviceBuffer<unsigned>(m);
  }
  k_ = DeviceBuffer<double>(m);
  err_ = DeviceBuffer<double>(m);
  dir_ = DeviceBuffer<double>(2 * m);
  r_ = DeviceBuffer<double>(m);
  split_ = DeviceBuffer<unsigned char>(m);
  part_k_ = DeviceBuffer<double>(nb);
  blk_sums_ = DeviceBuffer<double>(5 * nb);
  blk_counts_ = DeviceBuffer<unsigned>(5 * nb);
  blk_off_ = DeviceBuffer<unsigned>(nb);
  reserved_ = m;
}

// x0 < x1 and y0 < y1. `out` (or null) takes the partition in acceptance order; integrate()
// orders it.
Adapt2DResult ExprAdaptive2D::rounds(double x0, double x1, double y0, double y1,
                                     const Adapt2DOptions& opt, double* out, uint64_t cap) {
  hipStream_t s = stream_.get();
  const unsigned long long max_iv = opt.max_intervals;
  const unsigned max_depth = static_cast<unsigned>(opt.max_depth);
  const double box_x = x1 - x0, box_y = y1 - y0;
  double2* done = reinterpret_cast<double2*>(out);
  const unsigned long long done_cap = cap;
  unsigned long long* st = state_.get();
  unsigned long long* rec = record_.device_ptr();
  MIINT_HIP(hipMemsetAsync(st, 0, kStateWords * sizeof(unsigned long long), s));
  const unsigned long long px = opt.panels_x, py = opt.panels_y;
  unsigned long long n = px * py;
  int cur = 0;
  module_.launch(kInit, static_cast<unsigned>((n + kBlock - 1) / kBlock), 1, kBlock, s, x0, x1,
                 y0, y1, px, py, reinterpret_cast<double2*>(xs_[0].get()),
                 reinterpret_cast<double2*>(ys_[0].get()), depth_[0].get());
  Adapt2DResult r;
  for (;;) {
    MIINT_CHECK(n >= 1 && n <= max_iv && n <= reserved_,
                "adaptive 2-D: the active list left its bound");
    MIINT_CHECK(r.rounds <= 2 * static_cast<uint64_t>(opt.max_depth),
                "adaptive 2-D: more rounds than depths");
    const unsigned blocks = static_cast<unsigned>((n + kBlock - 1) / kBlock);
    const int nb = static_cast<int>(blocks);
    const double2* xs = reinterpret_cast<const double2*>(xs_[cur].get());
    const double2* ys = reinterpret_cast<const double2*>(ys_[cur].get());
    double2* dir = reinterpret_cast<double2*>(dir_.get());
    const unsigned* depth = depth_[cur].get();
    module_.launch(kEval, blocks, 1, kBlock, s, n, xs, ys, k_.get(), err_.get(), dir, r_.get(),
                   part_k_.get());
    module_.launch(kClose, 1, 1, kBlock, s, static_cast<const double*>(part_k_.get()), nb,
                   opt.rtol, opt.atol, st);
    module_.launch(kDecide, blocks, 1, kBlock, s, n, xs, ys,
                   static_cast<const double*>(k_.get()), static_cast<const double*>(err_.get()),
                   static_cast<const double2*>(dir), static_cast<const double*>(r_.get()), depth,
                   box_x, box_y, max_depth, static_cast<const unsigned long long*>(st),
                   split_.get(), blk_counts_.get(), blk_sums_.get());
    module_.launch(kPrefix, 1, 1, kBlock, s, nb, n, max_iv,
                   static_cast<const unsigned*>(blk_counts_.get()),
                   static_cast<const double*>(blk_sums_.get()), blk_off_.get(), st, rec);
    module_.launch(kScatter, blocks, 1, kBlock, s, n, xs, ys, depth,
                   static_cast<const unsigned char*>(split_.get()),
                   static_cast<const unsigned*>(blk_off_.get()),
                   static_cast<const unsigned long long*>(st),
                   reinterpret_cast<double2*>(xs_[cur ^ 1].get()),
                   reinterpret_cast<double2*>(ys_[cur ^ 1].get()), depth_[cur ^ 1].get(), max_iv,
                   done, done_cap);
    stream_.sync();
    ++r.rounds;
    r.evals += 225 * n;
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
  r.splits_x = record_[kSplitsX];
  r.splits_y = record_[kSplitsY];
  r.floor = record_[kFloor];
  r.forced = record_[kForced];
  r.nonfinite = record_[kNonfinite];
  r.capped = record_[kCapped] != 0;
  r.converged = r.err_est <= r.tol && !r.capped && r.nonfinite == 0;
  return r;
}

Adapt2DResult ExprAdaptive2D::integrate(double ax, double bx, double ay, double by,
                                        const Adapt2DOptions& opt, double* rects_out,
                                        uint64_t capacity) {
  adapt2d_check(ax, bx, ay, by, opt);
  MIINT_CHECK(rects_out == nullptr || capacity >= opt.max_intervals,
              "adaptive 2-D: rects_out holds " + std::to_string(capacity) +
                  " rectangles, fewer than max_intervals = " + std::to_string(opt.max_intervals));
  if (ax == bx || ay == by) {
    Adapt2DResult r;
    r.tol = opt.atol;
    r.converged = true;
    return r;
  }
  DeviceGuard g(device_);
  reserve(opt.max_intervals);
  const bool negate = (ax > bx) != (ay > by);
  e0_.record(stream_.get());
  Adapt2DResult r = rounds(std::min(ax, bx), std::max(ax, bx), std::min(ay, by),
                           std::max(ay, by), opt, rects_out, capacity);
  e1_.record(stream_.get());
  stream_.sync();
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  if (negate) r.value = -r.value;
  if (rects_out != nullptr) {
    // the rounds stored the partition in acceptance order. Not on the rounds' path: ordered on
    // the host by (y0, x0), every rectangle with x0 < x1 and y0 < y1 whatever the ends' order.
    MIINT_CHECK(r.intervals <= capacity, "adaptive 2-D: the partition passed rects_out");
    using Rect = std::array<double, 4>;
    std::vector<Rect> rc(r.intervals);
    MIINT_HIP(hipMemcpy(rc.data(), rects_out, rc.size() * 4 * sizeof(double),
                        hipMemcpyDeviceToHost));
    std::sort(rc.begin(), rc.end(), [](const Rect& p, const Rect& q) {
      return p[2] != q[2] ? p[2] < q[2] : p[0] < q[0];
    });
    MIINT_HIP(hipMemcpy(rects_out, rc.data(), rc.size() * 4 * sizeof(double),
                        hipMemcpyHostToDevice));
  }
  return r;
}

double ExprAdaptive2D::time(double ax, double bx, double ay, double by, const Adapt2DOptions& opt,
                            int iters) {
  MIINT_CHECK(iters >= 1, "bad adaptive 2-D timing request");
  adapt2d_check(ax, bx, ay, by, opt);
  if (ax == bx || ay == by) return 0.0;
  DeviceGuard g(device_);
  reserve(opt.max_intervals);
  const double x0 = std::min(ax, bx), x1 = std::max(ax, bx);
  const double y0 = std::min(ay, by), y1 = std::max(ay, by);
  return detail::time_enqueues(stream_, e0_, e1_, iters,
                               [&] { (void)rounds(x0, x1, y0, y1, opt, nullptr, 0); });
}

}  // namespace miint
