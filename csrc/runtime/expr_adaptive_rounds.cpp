// What the adaptive families share behind their rules (see miint/expr_rtc.hpp): the device text
// of a round's kernels, for intervals and for rectangles, and the host engine that runs the
// rounds, detail::AdaptRounds.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>

#include "miint/expr.hpp"

namespace miint {
namespace detail {

namespace {
constexpr int kBlock = 256;

// The device's totals: words 0..7 are doubles, 8.. counters (sixteen words for intervals, and
// splits_x, splits_y behind them for rectangles). _prefix stores the same words into the pinned
// record at the end of every round.
enum { kS, kE, kR, kTol, kSumK };
enum { kAccepted = 8, kSplits, kFloor, kForced, kNonfinite, kNext, kCapped, kBase, kSplitsX,
       kSplitsY };

std::string kernel_head(const std::string& name, const std::string& params) {
  return "extern \"C\" __global__ __launch_bounds__(256) void " + name + "(\n    " + params +
         ") {\n";
}

// What a round's kernels do per dimension, as device text: whole lines, passed into the one
// text of adapt_round_source.
struct RoundText {
  const char* name;            // the kernels' prefix
  int counters, words;         // per workgroup in blk_counts; in the state and the record
  const char* state;           // the comment on the state's words
  const char* init;            // the comment and the kernel of the first list
  const char* decide_comment;
  const char* decide_params;
  const char* classify;        // an item's `how` (and in 2-D its axis), then its split byte
  const char* count_more;      // _decide: the workgroup's counts behind the four common ones
  const char* store_more;      // _decide: their stores into bc[4..]
  const char* total_more;      // _prefix, thread 0: their totals from cnt[3..]
  const char* record_more;     // _prefix, thread 0: the state's words behind st[15]
  const char* scatter_comment;
  const char* scatter_params;
  const char* split_lane;      // sp: this lane's item is split
  const char* load;            // the item, for its children or for `done`
  const char* children;        // inside if (sp)
  const char* done;            // inside else if (done != nullptr), after q
};

const RoundText kIntervals = {
    "miint_adapt", 4, 16,
    R"(// st[0..7] as doubles: S_acc, E_acc, R_acc, tol, sum_K; st[8..15]: accepted, splits, floor,
// forced, nonfinite, next, capped, base (the intervals accepted before this round).
)",
    R"(// The first list: interval i of `panels` equal ones, edges a + ((b - a) i) / panels, the last b.
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
)",
    R"(// Per interval the decision (miint/expr.hpp has the order); per workgroup the number to split,
// the three counters and five sums: the accepted K, err and R, the K and err to be split.
)",
    R"(unsigned long long n, const double2* __restrict__ list, const double* __restrict__ k,
    const double* __restrict__ err, const double* __restrict__ r,
    const unsigned* __restrict__ depth, double width, unsigned max_depth,
    const unsigned long long* __restrict__ st, unsigned char* __restrict__ split,
    unsigned* __restrict__ blk_counts, double* __restrict__ blk_sums)",
    R"(  if (i < n) {
    const double2 iv = list[i];
    const double kv = k[i], ev = err[i], rv = r[i];
    const double w = iv.y - iv.x, c = iv.x + 0.5 * w;
    if (!(isfinite(kv) && isfinite(ev))) how = 1;
    else if (!(ev > (tol * w) / width)) how = 2;
    else if (ev <= 0x1.9p-47 * rv) how = 3;  // 50 * 2^-52
    else if (depth[i] >= max_depth || c == iv.x || c == iv.y) how = 4;
    else how = 5;
    split[i] = how == 5 ? 1 : 0;
)",
    "", "", "", "",
    R"(// Children (lo, c), (c, hi) at depth + 1 to slots 2 p, 2 p + 1 of the next list, p the number
// of intervals split before this one: blk_off plus the lanes before it in the workgroup
// (ballot and popcount per wave, the waves' counts through LDS). An accepted interval (all of
// them in a capped round) goes to slot base + (the accepted before it) of `done`, if given.
// Nothing is stored at or past next_cap or done_cap.
)",
    R"(unsigned long long n, const double2* __restrict__ list, const unsigned* __restrict__ depth,
    const unsigned char* __restrict__ split, const unsigned* __restrict__ blk_off,
    const unsigned long long* __restrict__ st, double2* __restrict__ next,
    unsigned* __restrict__ next_depth, unsigned long long next_cap, double2* __restrict__ done,
    unsigned long long done_cap)",
    "  const bool sp = valid && !capped && split[i] != 0;\n",
    "  const double2 iv = list[i];\n",
    R"(    const double c = iv.x + 0.5 * (iv.y - iv.x);
    const unsigned d = depth[i] + 1u;
    if (2ull * p + 1ull < next_cap) {
      next[2ull * p] = make_double2(iv.x, c);
      next[2ull * p + 1ull] = make_double2(c, iv.y);
      next_depth[2ull * p] = d;
      next_depth[2ull * p + 1ull] = d;
    }
)",
    "    if (q < done_cap) done[q] = iv;\n"};

const RoundText kRectangles = {
    "miint_adapt2d", 5, 18,
    R"(// st[0..7] as doubles: S_acc, E_acc, R_acc, tol, sum_K; st[8..17]: accepted, splits, floor,
// forced, nonfinite, next, capped, base (the rectangles accepted before this round), splits_x,
// splits_y.
)",
    R"(// The first list: rectangle i = iy * px + ix (x fastest) of px x py equal ones; per axis the
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
)",
    R"(// Per rectangle the axis and the decision (miint/expr.hpp has the order); per workgroup the
// number to split (and of those along x), the three counters and five sums: the accepted K,
// err and R, the K and err to be split. depth holds the x depth in its low half, the y depth
// in its high half. split: 0 accepted, 1 bisect x, 2 bisect y.
)",
    R"(unsigned long long n, const double2* __restrict__ xs, const double2* __restrict__ ys,
    const double* __restrict__ k, const double* __restrict__ err,
    const double2* __restrict__ dir, const double* __restrict__ r,
    const unsigned* __restrict__ depth, double box_x, double box_y, unsigned max_depth,
    const unsigned long long* __restrict__ st, unsigned char* __restrict__ split,
    unsigned* __restrict__ blk_counts, double* __restrict__ blk_sums)",
    R"(  bool along_x = false;
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
)",
    "  const int n_split_x = __syncthreads_count(how == 5 && along_x);\n",
    "    bc[4] = (unsigned)n_split_x;\n",
    "    const unsigned long long split_x = (cnt[3][0] + cnt[3][1]) + (cnt[3][2] + cnt[3][3]);\n",
    "    st[16] += capped ? 0ull : split_x;\n"
    "    st[17] += capped ? 0ull : total_split - split_x;\n",
    R"(// The two children of a rectangle bisected along its axis, that axis's depth + 1, to slots
// 2 p, 2 p + 1 of the next lists, p the number of rectangles split before this one: blk_off
// plus the lanes before it in the workgroup (ballot and popcount per wave, the waves' counts
// through LDS). An accepted rectangle (all of them in a capped round) goes to slot base + (the
// accepted before it) of `done`, if given, as (x0, x1), (y0, y1). Nothing is stored at or past
// next_cap or done_cap.
)",
    R"(unsigned long long n, const double2* __restrict__ xs, const double2* __restrict__ ys,
    const unsigned* __restrict__ depth, const unsigned char* __restrict__ split,
    const unsigned* __restrict__ blk_off, const unsigned long long* __restrict__ st,
    double2* __restrict__ next_xs, double2* __restrict__ next_ys,
    unsigned* __restrict__ next_depth, unsigned long long next_cap, double2* __restrict__ done,
    unsigned long long done_cap)",
    R"(  const unsigned char axis = valid && !capped ? split[i] : (unsigned char)0;
  const bool sp = axis != 0;
)",
    "  const double2 xr = xs[i], yr = ys[i];\n",
    R"(    if (2ull * p + 1ull < next_cap) {
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
)",
    R"(    if (q < done_cap) {
      done[2ull * q] = xr;
      done[2ull * q + 1ull] = yr;
    }
)"};

std::string round_kernel(int dims, const char* which) {
  return std::string((dims == 1 ? kIntervals : kRectangles).name) + which;
}
}  // namespace

std::string hex(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%a", v);
  return b;
}

std::string num(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.17g", v);
  return b;
}

double word_as_double(unsigned long long w) {
  double d;
  std::memcpy(&d, &w, sizeof d);
  return d;
}

void adapt_check_tolerances(const std::string& what, double rtol, double atol,
                            uint64_t max_intervals) {
  MIINT_CHECK(rtol >= 0.0 && atol >= 0.0 && std::isfinite(rtol) && std::isfinite(atol) &&
                  (rtol > 0.0 || atol > 0.0),
              what + "rtol = " + num(rtol) + " and atol = " + num(atol) +
                  " must be finite and >= 0, and not both 0");
  MIINT_CHECK(max_intervals >= 1 && max_intervals <= kAdaptMaxIntervalsLimit,
              what + "max_intervals = " + std::to_string(max_intervals) + " must be 1..2^26");
}

void adapt_check_depth(const std::string& what, int max_depth, const char* per) {
  MIINT_CHECK(max_depth >= 0 && max_depth <= kAdaptMaxDepthLimit,
              what + "max_depth = " + std::to_string(max_depth) + " must be 0..200" + per);
}

std::string adapt_eval_source(const std::string& comment, const std::string& name,
                              const std::string& params, const std::string& call,
                              const std::string& stores) {
  return comment + kernel_head(name, params) + R"(  __shared__ double red[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  double v = 0.0;
  if (i < n) {
)" + call + R"(    k[i] = v;
    err[i] = e;
)" + stores + R"(    r[i] = a;
  }
  MIINT_BLOCK_SUM(v, red);
  if (threadIdx.x == 0) part_k[blockIdx.x] = MIINT_RED(red);
}
)";
}

std::string adapt_round_source(int dims, const std::string& eval) {
  const RoundText& t = dims == 1 ? kIntervals : kRectangles;
  const std::string name = t.name, stride = std::to_string(t.counters) + "ull";
  // `line` once per counter behind the splits' own: '#' its number c, '@' its row c - 1 of cnt
  auto per_counter = [&](const std::string& line) {
    std::string s;
    for (int c = 1; c < t.counters; ++c)
      for (char ch : line)
        s += ch == '#' ? std::to_string(c) : ch == '@' ? std::to_string(c - 1) : std::string(1, ch);
    return s;
  };
  std::string src = "\n" + std::string(t.state) + R"(#define MIINT_ST_D(st, i) (((double*)(st))[i])

)" + t.init + "\n" + eval + R"(
// sum_K over the nb workgroups' partials, then the round's tolerance. A NaN sum gives a NaN
// tolerance (atol > NaN is false).
)" + kernel_head(name + "_close",
                R"(const double* __restrict__ part_k, int nb, double rtol, double atol,
    unsigned long long* __restrict__ st)") + R"(  double sum_k;
  MIINT_CLOSE(part_k, nb, 1.0, sum_k);
  if (threadIdx.x == 0) {
    const double t = rtol * fabs(MIINT_ST_D(st, 0) + sum_k);
    MIINT_ST_D(st, 4) = sum_k;
    MIINT_ST_D(st, 3) = atol > t ? atol : t;
  }
}

)" + t.decide_comment + kernel_head(name + "_decide", t.decide_params) +
                    R"(  __shared__ double red[5][4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const double tol = ((const double*)st)[3];
  double ak = 0.0, ae = 0.0, ar = 0.0, pk = 0.0, pe = 0.0;
  int how = 0;  // 1 nonfinite, 2 within tolerance, 3 floor, 4 forced, 5 split
)" + t.classify + R"(    if (how == 5) {
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
)" + t.count_more + R"(  MIINT_BLOCK_SUM(ak, red[0]);
  MIINT_BLOCK_SUM(ae, red[1]);
  MIINT_BLOCK_SUM(ar, red[2]);
  MIINT_BLOCK_SUM(pk, red[3]);
  MIINT_BLOCK_SUM(pe, red[4]);
  if (threadIdx.x == 0) {
    unsigned* bc = blk_counts + )" + stride + R"( * blockIdx.x;
    bc[0] = (unsigned)n_split;
    bc[1] = (unsigned)n_floor;
    bc[2] = (unsigned)n_forced;
    bc[3] = (unsigned)n_nonfinite;
)" + t.store_more + R"(    double* bs = blk_sums + 5ull * blockIdx.x;
    for (int q = 0; q < 5; ++q) bs[q] = MIINT_RED(red[q]);
  }
}

// One workgroup over the nb workgroups of the round. Thread t owns the contiguous run of
// per = ceil(nb / 256) of them from t * per: their sums in order, then the block reduction;
// thread 0 scans the 256 runs' split counts, and every thread writes its run's exclusive
// prefixes. Thread 0 then closes the round: capped or not, the totals, the record.
)" + kernel_head(name + "_prefix",
                R"(int nb, unsigned long long n, unsigned long long max_intervals,
    const unsigned* __restrict__ blk_counts, const double* __restrict__ blk_sums,
    unsigned* __restrict__ blk_off, unsigned long long* __restrict__ st,
    unsigned long long* __restrict__ record)") + R"(  __shared__ double red[5][4];
  __shared__ unsigned long long runs[256];
  __shared__ unsigned long long cnt[)" + std::to_string(t.counters - 1) + R"(][4];
  const int per = (nb + 255) / 256;
  const int first = (int)threadIdx.x * per;
  const int last = first + per < nb ? first + per : nb;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned long long n_split = 0)" + per_counter(", c# = 0") + R"(;
  for (int b = first; b < last; ++b) {
    for (int q = 0; q < 5; ++q) s[q] += blk_sums[5ull * b + q];
    n_split += blk_counts[)" + stride + R"( * b];
)" + per_counter("    c# += blk_counts[" + stride + " * b + #];\n") + R"(  }
  runs[threadIdx.x] = n_split;
  for (int o = 32; o > 0; o >>= 1) {
)" + per_counter("    c# += __shfl_xor(c#, o, 64);\n") + R"(  }
  if ((threadIdx.x & 63) == 0) {
)" + per_counter("    cnt[@][threadIdx.x >> 6] = c#;\n") + R"(  }
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
)" + t.total_more + R"(    const bool capped = accepted + (n - total_split) + 2ull * total_split > max_intervals;
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
)" + t.record_more + R"(    st[13] = capped ? 0ull : 2ull * total_split;
    st[14] = capped ? 1ull : 0ull;
    for (int q = 0; q < 8; ++q) MIINT_ST_D(record, q) = MIINT_ST_D(st, q);
    for (int q = 8; q < )" + std::to_string(t.words) + R"(; ++q) record[q] = st[q];
  }
  __syncthreads();
  unsigned long long off = runs[threadIdx.x];
  for (int b = first; b < last; ++b) {
    blk_off[b] = (unsigned)off;
    off += blk_counts[)" + stride + R"( * b];
  }
}

)" + t.scatter_comment + kernel_head(name + "_scatter", t.scatter_params) +
                    R"(  __shared__ unsigned waves[4];
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool capped = st[14] != 0ull;
  const bool valid = i < n;
)" + t.split_lane + R"(  const unsigned long long mask = __ballot(sp);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) waves[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  unsigned before = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  for (unsigned w = 0; w < wave; ++w) before += waves[w];
  if (!valid) return;
)" + t.load + R"(  const unsigned long long p = capped ? 0ull : (unsigned long long)blk_off[blockIdx.x] + before;
  if (sp) {
)" + t.children + R"(  } else if (done != nullptr) {
    const unsigned long long q = st[15] + (i - p);
)" + t.done + R"(  }
}
)";
  return src;
}

AdaptRounds::AdaptRounds(int dims, const std::string& code, const char* eval, int device)
    : dims_(dims), device_(device), what_(dims == 1 ? "adaptive" : "adaptive 2-D"),
      stream_((set_device(device), Stream())),
      module_(code, device, stream_,  // the names live until the module is loaded
              {round_kernel(dims, "_init").c_str(), eval, round_kernel(dims, "_close").c_str(),
               round_kernel(dims, "_decide").c_str(), round_kernel(dims, "_prefix").c_str(),
               round_kernel(dims, "_scatter").c_str()}) {
  DeviceGuard g(device);
  const size_t words = dims == 1 ? kSplitsX : kSplitsY + 1;
  state_ = DeviceBuffer<unsigned long long>(words);
  record_ = PinnedBuffer<unsigned long long>(words);
}

void AdaptRounds::reserve(uint64_t m) {
  if (m <= reserved_) return;
  stream_.sync();
  const uint64_t nb = (m + kBlock - 1) / kBlock;
  for (int q = 0; q < 2; ++q) {
    xs_[q] = DeviceBuffer<double>(2 * m);
    if (dims_ == 2) ys_[q] = DeviceBuffer<double>(2 * m);
    depth_[q] = DeviceBuffer<unsigned>(m);
  }
  k_ = DeviceBuffer<double>(m);
  err_ = DeviceBuffer<double>(m);
  if (dims_ == 2) dir_ = DeviceBuffer<double>(2 * m);
  r_ = DeviceBuffer<double>(m);
  split_ = DeviceBuffer<unsigned char>(m);
  part_k_ = DeviceBuffer<double>(nb);
  blk_sums_ = DeviceBuffer<double>(5 * nb);
  blk_counts_ = DeviceBuffer<unsigned>((dims_ == 1 ? 4 : 5) * nb);
  blk_off_ = DeviceBuffer<unsigned>(nb);
  reserved_ = m;
}

void AdaptRounds::check_capacity(const double* out, uint64_t capacity,
                                 uint64_t max_intervals) const {
  MIINT_CHECK(out == nullptr || capacity >= max_intervals,
              what_ + (dims_ == 1 ? ": intervals_out holds " : ": rects_out holds ") +
                  std::to_string(capacity) + (dims_ == 1 ? " intervals" : " rectangles") +
                  ", fewer than max_intervals = " + std::to_string(max_intervals));
}

template <class Result>
Result AdaptRounds::run(const AdaptJob& job, uint64_t evals_per, const Eval& eval) {
  hipStream_t s = stream_.get();
  const bool two = dims_ == 2;
  const unsigned long long max_iv = job.max_intervals, done_cap = job.capacity;
  const unsigned max_depth = static_cast<unsigned>(job.max_depth);
  const double box_x = job.x1 - job.x0, box_y = job.y1 - job.y0;
  double2* done = reinterpret_cast<double2*>(job.out);
  unsigned long long* st = state_.get();
  unsigned long long* rec = record_.device_ptr();
  auto pairs = [](DeviceBuffer<double>& b) { return reinterpret_cast<double2*>(b.get()); };
  MIINT_HIP(hipMemsetAsync(st, 0, state_.size() * sizeof(unsigned long long), s));
  const unsigned long long px = job.px, py = job.py;
  unsigned long long n = two ? px * py : px;
  int cur = 0;
  const unsigned first = static_cast<unsigned>((n + kBlock - 1) / kBlock);
  if (two)
    module_.launch(kInit, first, 1, kBlock, s, job.x0, job.x1, job.y0, job.y1, px, py,
                   pairs(xs_[0]), pairs(ys_[0]), depth_[0].get());
  else
    module_.launch(kInit, first, 1, kBlock, s, job.x0, job.x1, px, pairs(xs_[0]),
                   depth_[0].get());
  Result r;
  for (;;) {
    MIINT_CHECK(n >= 1 && n <= max_iv && n <= reserved_,
                what_ + ": the active list left its bound");
    MIINT_CHECK(r.rounds <= static_cast<uint64_t>(dims_) * static_cast<uint64_t>(job.max_depth),
                what_ + ": more rounds than depths");
    const unsigned blocks = static_cast<unsigned>((n + kBlock - 1) / kBlock);
    const int nb = static_cast<int>(blocks);
    const double2* xs = pairs(xs_[cur]);
    const double2* ys = two ? pairs(ys_[cur]) : nullptr;
    double2* dir = two ? pairs(dir_) : nullptr;
    const unsigned* depth = depth_[cur].get();
    const double *k = k_.get(), *err = err_.get(), *rr = r_.get();
    eval(AdaptItems{s, blocks, n, xs, ys, depth, k_.get(), err_.get(), r_.get(), dir,
                    part_k_.get()});
    module_.launch(kClose, 1, 1, kBlock, s, static_cast<const double*>(part_k_.get()), nb,
                   job.rtol, job.atol, st);
    if (two)
      module_.launch(kDecide, blocks, 1, kBlock, s, n, xs, ys, k, err,
                     static_cast<const double2*>(dir), rr, depth, box_x, box_y, max_depth,
                     static_cast<const unsigned long long*>(st), split_.get(), blk_counts_.get(),
                     blk_sums_.get());
    else
      module_.launch(kDecide, blocks, 1, kBlock, s, n, xs, k, err, rr, depth, box_x, max_depth,
                     static_cast<const unsigned long long*>(st), split_.get(), blk_counts_.get(),
                     blk_sums_.get());
    module_.launch(kPrefix, 1, 1, kBlock, s, nb, n, max_iv,
                   static_cast<const unsigned*>(blk_counts_.get()),
                   static_cast<const double*>(blk_sums_.get()), blk_off_.get(), st, rec);
    const unsigned char* split = split_.get();
    const unsigned* blk_off = blk_off_.get();
    if (two)
      module_.launch(kScatter, blocks, 1, kBlock, s, n, xs, ys, depth, split, blk_off,
                     static_cast<const unsigned long long*>(st), pairs(xs_[cur ^ 1]),
                     pairs(ys_[cur ^ 1]), depth_[cur ^ 1].get(), max_iv, done, done_cap);
    else
      module_.launch(kScatter, blocks, 1, kBlock, s, n, xs, depth, split, blk_off,
                     static_cast<const unsigned long long*>(st), pairs(xs_[cur ^ 1]),
                     depth_[cur ^ 1].get(), max_iv, done, done_cap);
    stream_.sync();
    ++r.rounds;
    r.evals += evals_per * n;
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
  if constexpr (std::is_same<Result, Adapt2DResult>::value) {
    r.splits_x = record_[kSplitsX];
    r.splits_y = record_[kSplitsY];
  }
  r.floor = record_[kFloor];
  r.forced = record_[kForced];
  r.nonfinite = record_[kNonfinite];
  r.capped = record_[kCapped] != 0;
  r.converged = r.err_est <= r.tol && !r.capped && r.nonfinite == 0;
  return r;
}

template <class Result>
Result AdaptRounds::integrate(const AdaptJob& job, uint64_t evals_per, const Eval& eval) {
  e0_.record(stream_.get());
  Result r = run<Result>(job, evals_per, eval);
  e1_.record(stream_.get());
  stream_.sync();
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  if (job.out != nullptr) order(job, r.intervals);
  return r;
}

template AdaptResult AdaptRounds::run<AdaptResult>(const AdaptJob&, uint64_t, const Eval&);
template Adapt2DResult AdaptRounds::run<Adapt2DResult>(const AdaptJob&, uint64_t, const Eval&);
template AdaptResult AdaptRounds::integrate<AdaptResult>(const AdaptJob&, uint64_t, const Eval&);
template Adapt2DResult AdaptRounds::integrate<Adapt2DResult>(const AdaptJob&, uint64_t,
                                                             const Eval&);

namespace {
// `count` items of `out` to the host, put in order there, and back.
template <class Item, class Order>
void order_on_host(double* out, uint64_t count, Order&& in_order) {
  std::vector<Item> items(count);
  MIINT_HIP(hipMemcpy(items.data(), out, count * sizeof(Item), hipMemcpyDeviceToHost));
  in_order(items);
  MIINT_HIP(hipMemcpy(out, items.data(), count * sizeof(Item), hipMemcpyHostToDevice));
}
}  // namespace

// The rounds stored the partition in acceptance order. Not on the rounds' path: ordered on the
// host. Intervals are disjoint, so the order of their lower ends is the x order; rectangles go
// by (y0, x0), every one with x0 < x1 and y0 < y1 whatever the ends' order.
void AdaptRounds::order(const AdaptJob& job, uint64_t count) {
  MIINT_CHECK(count <= job.capacity, what_ + ": the partition passed " +
                                         (dims_ == 1 ? "intervals_out" : "rects_out"));
  if (dims_ == 1)
    order_on_host<std::pair<double, double>>(job.out, count, [&](auto& iv) {
      std::sort(iv.begin(), iv.end());
      if (!job.descending) return;
      std::reverse(iv.begin(), iv.end());
      for (auto& p : iv) std::swap(p.first, p.second);
    });
  else
    order_on_host<std::array<double, 4>>(job.out, count, [](auto& rc) {
      std::sort(rc.begin(), rc.end(), [](const auto& p, const auto& q) {
        return p[2] != q[2] ? p[2] < q[2] : p[0] < q[0];
      });
    });
}

}  // namespace detail
}  // namespace miint
