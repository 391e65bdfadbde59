// Integrals of a run-time f(x0, ..., x15) over a box by a randomly shifted rank-1 lattice rule
// (see miint/expr.hpp, ExprLattice).
#include <algorithm>
#include <cmath>
#include <limits>

#include "miint/expr.hpp"
#include "miint/integrator.hpp"

namespace miint {

namespace {
constexpr int kLatticeBlock = 256;
enum { kPartials, kClose, kFinish };  // module_'s kernels

// The Korobov multipliers a of m = kLatticeBuiltinMin..kLatticeBuiltinMax, as
// tools/lattice_search.py prints them (64 candidates congruent to 3 or 5 mod 8, seed 2024, the
// least e^2 over 16 dimensions with weights 1 / (j + 1)^2).
constexpr uint64_t kKorobovA[kLatticeBuiltinMax - kLatticeBuiltinMin + 1] = {
    389u,       // m = 10: e2 = 5.312470e-03
    109u,       // m = 11: e2 = 2.114894e-03
    3029u,      // m = 12: e2 = 9.571972e-04
    4781u,      // m = 13: e2 = 3.666836e-04
    7451u,      // m = 14: e2 = 1.420467e-04
    22757u,     // m = 15: e2 = 5.836251e-05
    54571u,     // m = 16: e2 = 2.293813e-05
    28997u,     // m = 17: e2 = 1.073511e-05
    78003u,     // m = 18: e2 = 3.994330e-06
    157773u,    // m = 19: e2 = 1.601344e-06
    351453u,    // m = 20: e2 = 6.156888e-07
    873187u,    // m = 21: e2 = 2.044632e-07
    2942315u,   // m = 22: e2 = 9.598285e-08
    6013717u,   // m = 23: e2 = 4.148354e-08
    10407029u,  // m = 24: e2 = 1.272788e-08
    16116915u,  // m = 25: e2 = 5.369906e-09
    55102557u,  // m = 26: e2 = 2.004781e-09
};

// What the kernels take by value: uniform, so it sits in scalar registers. The generated
// source declares the same layout.
struct RuleArgs {
  unsigned step[kLatticeMaxDim];  // z_j << (32 - m)
  unsigned z[kLatticeMaxDim];
  double a[kLatticeMaxDim];
  double w[kLatticeMaxDim];       // b_j - a_j
};

int checked_dim(int d) {
  MIINT_CHECK(d >= 1 && d <= kLatticeMaxDim,
              "lattice: d = " + std::to_string(d) + " must be 1.." + std::to_string(kLatticeMaxDim));
  return d;
}
int checked_grid(int grid) {
  MIINT_CHECK(grid >= 0 && grid <= kLatticeMaxGrid,
              "lattice: grid = " + std::to_string(grid) + " must be 0 (auto) ..2048");
  return grid;
}
void check_m(int m) {
  MIINT_CHECK(m >= kLatticeMinM && m <= kLatticeMaxM,
              "lattice: m = " + std::to_string(m) + " must be 2..30");
}
int shift_rows(const LatticeOptions& opt, int d) {
  if (opt.shift_words.empty()) {
    MIINT_CHECK(opt.shifts >= 1 && opt.shifts <= kLatticeMaxShifts,
                "lattice: shifts = " + std::to_string(opt.shifts) + " must be 1..4096");
    return opt.shifts;
  }
  const size_t words = opt.shift_words.size();
  MIINT_CHECK(words % d == 0 && words / d <= static_cast<size_t>(kLatticeMaxShifts),
              "lattice: " + std::to_string(words) + " shift words are not 1..4096 rows of d = " +
                  std::to_string(d));
  return static_cast<int>(words / d);
}
void check_box(const LatticeBox& box, double scale) {
  checked_dim(static_cast<int>(box.size()));
  for (size_t j = 0; j < box.size(); ++j)
    MIINT_CHECK(std::isfinite(box[j].first) && std::isfinite(box[j].second) &&
                    std::isfinite(box[j].second - box[j].first),
                "lattice: side " + std::to_string(j) + " of the box, [" +
                    std::to_string(box[j].first) + ", " + std::to_string(box[j].second) +
                    "], must be finite, and its width too");
  MIINT_CHECK(std::isfinite(scale), "lattice: scale = " + std::to_string(scale) + " must be finite");
}
}  // namespace

uint64_t lattice_multiplier(int m) {
  MIINT_CHECK(m >= kLatticeBuiltinMin && m <= kLatticeBuiltinMax,
              "lattice: no built-in generating vector for m = " + std::to_string(m) +
                  " (the table covers " + std::to_string(kLatticeBuiltinMin) + ".." +
                  std::to_string(kLatticeBuiltinMax) + "): pass z");
  return kKorobovA[m - kLatticeBuiltinMin];
}

std::vector<uint64_t> lattice_generator(int m, int d) {
  checked_dim(d);
  const uint64_t a = lattice_multiplier(m), mask = (1ull << m) - 1;
  std::vector<uint64_t> z(d);
  uint64_t p = 1;
  for (int j = 0; j < d; ++j, p = (p * a) & mask) z[j] = p;  // p, a < 2^30
  return z;
}

std::vector<uint32_t> lattice_shifts(uint64_t seed, int shifts, int d) {
  checked_dim(d);
  MIINT_CHECK(shifts >= 1 && shifts <= kLatticeMaxShifts,
              "lattice: shifts = " + std::to_string(shifts) + " must be 1..4096");
  std::vector<uint32_t> out(static_cast<size_t>(shifts) * d);
  for (int r = 0; r < shifts; ++r)
    for (int j = 0; j < d; ++j) {
      const uint64_t q = static_cast<uint64_t>(r) * kLatticeMaxDim + j;
      uint64_t z = seed + (q + 1) * 0x9E3779B97F4A7C15ull;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      out[static_cast<size_t>(r) * d + j] = static_cast<uint32_t>(z >> 32);
    }
  return out;
}

void lattice_check(const LatticeBox& box, int m, const LatticeOptions& opt, uint64_t begin,
                   uint64_t count, double scale) {
  check_box(box, scale);
  const int d = static_cast<int>(box.size());
  check_m(m);
  shift_rows(opt, d);
  const uint64_t n = 1ull << m;
  if (opt.z.empty()) {
    (void)lattice_multiplier(m);
  } else {
    MIINT_CHECK(opt.z.size() == box.size(), "lattice: " + std::to_string(opt.z.size()) +
                                                " generating entries for d = " + std::to_string(d));
    for (int j = 0; j < d; ++j)
      MIINT_CHECK(opt.z[j] % 2 == 1 && opt.z[j] < n,
                  "lattice: z[" + std::to_string(j) + "] = " + std::to_string(opt.z[j]) +
                      " must be odd and below n = " + std::to_string(n));
  }
  MIINT_CHECK(begin + count >= begin && begin + count <= n,
              "lattice: slice [" + std::to_string(begin) + ", " + std::to_string(begin) + " + " +
                  std::to_string(count) + ") outside [0, " + std::to_string(n) + ")");
}

namespace {
int walk_top(const LatticeOptions& opt) {
  return opt.m_max <= 0 ? kLatticeBuiltinMax : std::min(opt.m_max, kLatticeBuiltinMax);
}
}  // namespace

void lattice_check_walk(const LatticeBox& box, const LatticeOptions& opt, double scale) {
  check_box(box, scale);
  shift_rows(opt, static_cast<int>(box.size()));
  MIINT_CHECK(std::isfinite(opt.rtol) && std::isfinite(opt.atol) && opt.rtol >= 0 &&
                  opt.atol >= 0 && (opt.rtol > 0 || opt.atol > 0),
              "lattice: rtol = " + std::to_string(opt.rtol) + " and atol = " +
                  std::to_string(opt.atol) + " must be finite and >= 0, and not both 0");
  MIINT_CHECK(opt.z.empty(), "lattice: a walk over m takes the built-in vectors (z belongs to "
                             "one m)");
  const int top = walk_top(opt);
  MIINT_CHECK(opt.m_min >= kLatticeBuiltinMin && opt.m_min <= top,
              "lattice: m_min = " + std::to_string(opt.m_min) + " must lie in " +
                  std::to_string(kLatticeBuiltinMin) + "..m_max = " + std::to_string(top));
}

LatticeShape lattice_shape(uint64_t count, int shifts, int grid) {
  MIINT_CHECK(shifts >= 1 && shifts <= kLatticeMaxShifts,
              "lattice: shifts = " + std::to_string(shifts) + " must be 1..4096");
  checked_grid(grid);
  LatticeShape s;
  if (grid > 0) {
    s.gx = grid;
  } else {
    const uint64_t per_wg = kLatticeBlock * kLatticeMinPointsPerLane;
    const uint64_t want = count / per_wg + (count % per_wg ? 1 : 0);
    s.gx = static_cast<int>(std::min<uint64_t>(std::max<uint64_t>(want, 1), kLatticeMaxGrid));
  }
  s.gy = std::min(std::max(kLatticeMaxGrid / s.gx, 1), shifts);
  return s;
}

std::string expr_lattice_source(const std::string& expr, int d, bool periodic) {
  detail::expr_check_named(expr);
  checked_dim(d);
  // per dimension: the signature, the uniform sides, the lane's first fractions, a row's
  // start, a sample's coordinates and the step to the next point
  std::string sig, sides, first, row, at, adv;
  for (int j = 0; j < d; ++j) {
    const std::string J = std::to_string(j);
    sig += std::string(j ? ", " : "") + "double x" + J;
    sides += "  const double a" + J + " = rule.a[" + J + "], w" + J + " = rule.w[" + J + "];\n" +
             "  const unsigned s" + J + " = rule.step[" + J + "];\n";
    first += "  const unsigned b" + J + " = (unsigned)(((i_first * (unsigned long long)rule.z[" +
             J + "]) & mask) << up);\n";
    row += "    unsigned u" + J + " = b" + J + " + sh[" + J + "];\n";
    at += std::string(j ? ", " : "") + "fma(miint_lattice_t(u" + J + "), w" + J + ", a" + J + ")";
    adv += " u" + J + " += s" + J + ";";
  }
  const std::string unit =
      periodic ? "  return fma((double)u, 0x1p-32, 0x1p-33);\n"
               : "  const unsigned s = (unsigned)((int)u >> 31);\n"
                 "  const unsigned w = (u ^ s) & 0x7FFFFFFFu;\n"
                 "  return fma((double)w, 0x1p-31, 0x1p-32);\n";
  return std::string(detail::kRtcPrelude) + R"(
__device__ __forceinline__ double miint_fl()" + sig + R"() { return ()" + expr + R"(); }
// The unit coordinate of a 32-bit fraction, strictly inside (0, 1) and exact in fp64: the tent
// 1 - |2 tau - 1| of tau = (u + 1/2) / 2^32, or tau itself for a periodic rule.
__device__ __forceinline__ double miint_lattice_t(unsigned u) {
)" + unit + R"(}
#define MIINT_LATTICE_AT() miint_fl()" + at + R"()
#define MIINT_LATTICE_NEXT() do {)" + adv + R"( } while (0)

// Uniform for the whole launch, passed by value: scalar registers.
struct MiintLatticeRule {
  unsigned step[16];  // z_j << (32 - m): adding it wraps at 2^32, which is the mod n
  unsigned z[16];
  double a[16];
  double w[16];       // b_j - a_j
};

// gridDim.x point slices x gridDim.y shift lanes: workgroup (bx, by) walks shifts by,
// by + gridDim.y, ... below `rows`. A lane owns a contiguous run of the `count` points from i0
// (miint_lane_share). b_j, its first point's fraction without a shift, comes from the full
// 64-bit product (i0 + start) * z_j (both below 2^30), once per lane. Per shift the fractions
// start at b_j + shift[r][j]; after that a point is one 32-bit add per dimension. Four
// accumulators, four points per trip so their chains overlap. One partial per (shift, bx) at
// partials[r * gridDim.x + bx]. The shift words are workgroup-uniform reads (never written
// here). No workgroup waits on another.
extern "C" __global__ __launch_bounds__(256) void miint_lattice_partials(
    MiintLatticeRule rule, unsigned m, unsigned long long i0, unsigned long long count,
    const unsigned* __restrict__ shifts, unsigned rows, double* __restrict__ partials) {
  __shared__ double red[2][4];  // alternating per shift: one barrier per shift is enough
  unsigned long long start;
  const unsigned cnt = miint_lane_share(count, &start);
  const unsigned long long i_first = i0 + start;
  const unsigned long long mask = (1ull << m) - 1ull;
  const unsigned up = 32u - m;
)" + sides + first + R"(  unsigned par = 0;
  for (unsigned r = blockIdx.y; r < rows; r += gridDim.y, par ^= 1u) {
    const unsigned* __restrict__ sh = shifts + (unsigned long long)r * )" + std::to_string(d) + R"(u;
)" + row + R"(    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    unsigned c = 0;
    for (; c + 4 <= cnt; c += 4) {
      acc0 += MIINT_LATTICE_AT(); MIINT_LATTICE_NEXT();
      acc1 += MIINT_LATTICE_AT(); MIINT_LATTICE_NEXT();
      acc2 += MIINT_LATTICE_AT(); MIINT_LATTICE_NEXT();
      acc3 += MIINT_LATTICE_AT(); MIINT_LATTICE_NEXT();
    }
    for (; c < cnt; ++c) {
      acc0 += MIINT_LATTICE_AT(); MIINT_LATTICE_NEXT();
    }
    double acc = (acc0 + acc1) + (acc2 + acc3);
    MIINT_BLOCK_SUM(acc, red[par]);
    if (threadIdx.x == 0)
      partials[(unsigned long long)r * gridDim.x + blockIdx.x] = MIINT_RED(red[par]);
  }
}

// One workgroup per shift closes its gx partials: sums[r] = S_r of this launch's points.
extern "C" __global__ __launch_bounds__(256) void miint_lattice_close(
    const double* __restrict__ partials, int gx, unsigned rows, double* __restrict__ sums) {
  const unsigned r = blockIdx.x;
  if (r >= rows) return;
  const double* row = partials + (unsigned long long)r * (unsigned)gx;
  MIINT_CLOSE(row, gx, 1.0, sums[r]);
}

// One workgroup: est_r = (c * S_r) * inv_n (c = vol * scale, inv_n = 2^-m), then thread 0 forms
// value = (sum est_r) / R and err_est = sqrt(sum (est_r - value)^2 / (R (R - 1))) in index
// order (+inf for R = 1). out is pinned host memory: [0] value, [1] err_est, [2 + r] est_r.
extern "C" __global__ __launch_bounds__(256) void miint_lattice_finish(
    const double* __restrict__ sums, unsigned rows, double c, double inv_n,
    double* __restrict__ out) {
  __shared__ double est[4096];
  for (unsigned r = threadIdx.x; r < rows; r += 256) {
    const double e = (c * sums[r]) * inv_n;
    est[r] = e;
    out[2 + r] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (unsigned r = 0; r < rows; ++r) s += est[r];
    const double value = s / (double)rows;
    double q = 0.0;
    for (unsigned r = 0; r < rows; ++r) q += (est[r] - value) * (est[r] - value);
    out[0] = value;
    out[1] = rows > 1 ? sqrt(q / ((double)rows * (double)(rows - 1))) : __builtin_huge_val();
  }
}
)";
}

std::string expr_lattice_compile(const std::string& expr, int d, bool periodic) {
  return detail::rtc_compile_cached(expr_lattice_source(expr, d, periodic), expr);
}

// One call's numbers, checked and ready to launch.
struct ExprLattice::Plan {
  RuleArgs rule{};
  unsigned m = 0;
  uint64_t n = 0, begin = 0, count = 0;
  int rows = 0;
  std::vector<uint32_t> words;  // rows x d
  LatticeShape shape;
  double vol_scale = 0.0, inv_n = 0.0;
  bool empty_box = false;  // some a_j == b_j: nothing to launch
};

ExprLattice::ExprLattice(const std::string& expr, int d, bool periodic, int device, int grid)
    : expr_(expr), d_(checked_dim(d)), periodic_(periodic), device_(device),
      grid_(checked_grid(grid)), stream_((set_device(device), Stream())),
      module_(expr_lattice_compile(expr, d, periodic), device, stream_,
              {"miint_lattice_partials", "miint_lattice_close", "miint_lattice_finish"}) {
  DeviceGuard g(device);
  sums_ = DeviceBuffer<double>(kLatticeMaxShifts);
  host_out_ = PinnedBuffer<double>(2 + kLatticeMaxShifts);
}

void ExprLattice::use_partials(double* device_ptr, uint64_t capacity) {
  user_partials_ = device_ptr;
  user_capacity_ = device_ptr ? capacity : 0;
}

ExprLattice::Plan ExprLattice::plan(const LatticeBox& box, int m, const LatticeOptions& opt,
                                    uint64_t begin, uint64_t count, double scale) const {
  MIINT_CHECK(static_cast<int>(box.size()) == d_,
              "lattice: a box of " + std::to_string(box.size()) + " sides for an expression "
              "compiled for d = " + std::to_string(d_));
  check_m(m);
  if (count == ~0ull) count = (1ull << m) - std::min<uint64_t>(begin, 1ull << m);
  lattice_check(box, m, opt, begin, count, scale);
  Plan p;
  p.m = static_cast<unsigned>(m);
  p.n = 1ull << m;
  p.begin = begin;
  p.count = count;
  p.rows = shift_rows(opt, d_);
  p.words = opt.shift_words.empty() ? lattice_shifts(opt.seed, p.rows, d_) : opt.shift_words;
  const std::vector<uint64_t> z = opt.z.empty() ? lattice_generator(m, d_) : opt.z;
  double vol = 1.0;
  for (int j = 0; j < d_; ++j) {
    p.rule.z[j] = static_cast<unsigned>(z[j]);
    p.rule.step[j] = static_cast<unsigned>(z[j]) << (32 - m);
    p.rule.a[j] = box[j].first;
    p.rule.w[j] = box[j].second - box[j].first;
    vol *= p.rule.w[j];
    if (p.rule.w[j] == 0.0) p.empty_box = true;
  }
  p.vol_scale = vol * scale;
  p.inv_n = std::ldexp(1.0, -m);
  p.shape = lattice_shape(count, p.rows, grid_);
  p.shape.gy = std::min(p.shape.gy, p.rows);
  const uint64_t need = static_cast<uint64_t>(p.rows) * p.shape.gx;
  MIINT_CHECK(!user_partials_ || user_capacity_ >= need,
              "lattice: the caller's partials buffer holds " + std::to_string(user_capacity_) +
                  " doubles, fewer than shifts x gx = " + std::to_string(p.rows) + " x " +
                  std::to_string(p.shape.gx));
  return p;
}

// The shift words go to the device through pinned memory; the object's buffers grow to the
// largest call seen.
void ExprLattice::upload(const Plan& p, hipStream_t s) {
  const size_t words = p.words.size();
  if (shifts_.size() < words) {
    shifts_ = DeviceBuffer<unsigned>(words);
    host_shifts_ = PinnedBuffer<unsigned>(words);
  }
  const size_t need = static_cast<size_t>(p.rows) * p.shape.gx;
  if (!user_partials_ && partials_.size() < need) partials_ = DeviceBuffer<double>(need);
  std::copy(p.words.begin(), p.words.end(), host_shifts_.get());
  MIINT_HIP(hipMemcpyAsync(shifts_.get(), host_shifts_.get(), words * sizeof(unsigned),
                           hipMemcpyHostToDevice, s));
}

void ExprLattice::enqueue(const Plan& p, const Comm* comm, hipStream_t s) {
  double* partials = user_partials_ ? user_partials_ : partials_.get();
  const unsigned rows = static_cast<unsigned>(p.rows);
  module_.launch(kPartials, p.shape.gx, p.shape.gy, kLatticeBlock, s, p.rule, p.m,
                 static_cast<unsigned long long>(p.begin),
                 static_cast<unsigned long long>(p.count),
                 static_cast<const unsigned*>(shifts_.get()), rows, partials);
  module_.launch(kClose, rows, 1, kLatticeBlock, s, static_cast<const double*>(partials),
                 p.shape.gx, rows, sums_.get());
  if (comm && comm->world() > 1) comm->allreduce_sum(sums_.get(), sums_.get(), rows, s);
  module_.launch(kFinish, 1, 1, kLatticeBlock, s, static_cast<const double*>(sums_.get()), rows,
                 p.vol_scale, p.inv_n, host_out_.device_ptr());
}

LatticeResult ExprLattice::integrate(const LatticeBox& box, int m, const LatticeOptions& opt,
                                     uint64_t begin, uint64_t count, double scale,
                                     const Comm* comm) {
  const Plan p = plan(box, m, opt, begin, count, scale);
  LatticeResult r;
  r.m = m;
  r.n = p.n;
  r.shifts = p.rows;
  r.evals = static_cast<uint64_t>(p.rows) * p.count;
  if (p.empty_box) {  // a_j == b_j: the volume is 0, on every rank alike
    r.estimates.assign(p.rows, 0.0);
    r.evals = 0;
    r.err_est = p.rows > 1 ? 0.0 : std::numeric_limits<double>::infinity();
    return r;
  }
  DeviceGuard g(device_);
  hipStream_t s = stream_.get();
  upload(p, s);
  e0_.record(s);
  enqueue(p, comm, s);
  e1_.record(s);
  stream_.sync();
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  r.value = host_out_[0];
  r.err_est = host_out_[1];
  r.estimates.assign(host_out_.get() + 2, host_out_.get() + 2 + p.rows);
  return r;
}

LatticeResult ExprLattice::integrate_to(const LatticeBox& box, const LatticeOptions& opt,
                                        double scale, const Comm* comm) {
  lattice_check_walk(box, opt, scale);
  LatticeOptions level = opt;
  if (level.shift_words.empty())  // the same shifts at every level
    level.shift_words = lattice_shifts(opt.seed, opt.shifts, d_);
  const int rank = comm ? comm->rank() : 0, world = comm ? comm->world() : 1;
  LatticeResult r;
  uint64_t evals = 0;
  int levels = 0;
  double ms = 0.0;
  for (int m = opt.m_min; m <= walk_top(opt); ++m) {
    uint64_t b = 0, c = 0;
    rank_slice(1ull << m, rank, world, &b, &c);
    r = integrate(box, m, level, b, c, scale, comm);
    evals += static_cast<uint64_t>(r.shifts) << m;
    ms += r.device_ms;
    ++levels;
    const double want = opt.rtol * std::fabs(r.value);
    if (r.err_est <= (opt.atol > want ? opt.atol : want)) {
      r.converged = true;
      break;
    }
  }
  r.evals = evals;
  r.levels = levels;
  r.device_ms = ms;
  return r;
}

double ExprLattice::time(const LatticeBox& box, int m, const LatticeOptions& opt, uint64_t begin,
                         uint64_t count, int iters, const std::function<void()>& at_start,
                         const std::function<void()>& at_end) {
  MIINT_CHECK(iters >= 1, "bad lattice timing request");
  const Plan p = plan(box, m, opt, begin, count, 1.0);
  MIINT_CHECK(!p.empty_box, "lattice: nothing to time on a box with an empty side");
  DeviceGuard g(device_);
  hipStream_t s = stream_.get();
  upload(p, s);
  return detail::time_enqueues(stream_, e0_, e1_, iters, [&] { enqueue(p, nullptr, s); },
                               at_start, at_end);
}

}  // namespace miint
