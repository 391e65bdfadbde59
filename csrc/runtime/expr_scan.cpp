// Running integral of a runtime integrand: F_i = scale * h * sum_{j <= i} f(x_j) on the
// sample grid, reduce-then-scan on the computed samples (see miint/expr.hpp, ExprScan).
//
// The slice's tiles are dealt to at most 2048 workgroups in contiguous runs of R tiles
// (expr_scan_shape). Association of one written value, exactly (every + below is one fp64
// addition):
//
//   S[t]   = four accumulators a_j = v_j + v_{j+4} + v_{j+8} + v_{j+12}, (a_0 + a_1) +
//            (a_2 + a_3), wave64 butterfly (__shfl_xor 32 .. 1), (r_0 + r_1) + (r_2 + r_3)
//   L[t]   = ((S[t_b] + S[t_b+1]) + ...) + S[t-1] the tiles before t in t's run, in order;
//            A[b] = the same sum over all of run b
//   B[b]   = (wb' + exc') (+ A[2u] for the second run of prefix thread u): a wave64 inclusive
//            scan over the 1024 prefix threads' sums of their (at most two) runs, then the
//            lower waves' totals in order; T = ((wt'_0 + wt'_1) + ...) + wt'_15
//   P[t]   = B[t / R] + L[t]
//   run_k  = ((v_0 + v_1) + ...) + v_k            the thread's 16 consecutive samples, in order
//   inc    = wave64 inclusive scan of the threads' run_15 (Hillis-Steele over __shfl_up:
//            inc += up(inc, 1), up(inc, 2), ..., up(inc, 32)); exc = up(inc, 1), 0 in lane 0
//   wb     = ((wt_0 + wt_1) + ...) + wt_{w-1}     the totals of the workgroup's lower waves
//   C      = ((T_0 + T_1) + ...) + T_{r-1}        the lower ranks' slice sums, rank order
//   F      = (((C + P[t]) + (wb + exc)) + run_k) * (h * scale)
//
// total = (T_0 + T_1 + ... in rank order) * (h * scale), formed on the host from the
// gathered T (one T without a communicator).
#include <algorithm>

#include "miint/expr.hpp"
#include "miint/trainscan.hpp"

namespace miint {

namespace {
constexpr int kScanBlock = 256;
constexpr int kPrefixBlock = 1024;
enum { kSums, kPrefix, kWrite };  // module_'s kernels
}  // namespace

std::string expr_scan_source(const std::string& expr) {
  expr_check(expr);
  return std::string(detail::kRtcPrelude) + R"(
typedef unsigned long long u64;
typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double miint_f(double x) { return ()" + expr + R"(); }

// The 16 consecutive samples of this thread, from slice-local sample g. The index goes
// u64 -> fp64 once, then += 1.0 (exact below 2^52): x = fma(idx, h, a) has the bits
// miint_expr_partials gives the sample. Samples at or past `lim` are 0 and not evaluated.
__device__ __forceinline__ void miint_items(double a, double h, double off, u64 i0, u64 g,
                                            u64 lim, double (&v)[16]) {
  double idx = (double)(i0 + g) + off;
  if (g + 16 <= lim) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      v[k] = miint_f(fma(idx, h, a));
      idx += 1.0;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      v[k] = 0.0;
      if (g + k < lim) v[k] = miint_f(fma(idx, h, a));
      idx += 1.0;
    }
  }
}

// Wave64 inclusive scan in lane order; *exc = the exclusive value (0 in lane 0).
__device__ __forceinline__ double miint_wave_scan(double x, int lane, double* exc) {
  double inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  const double e = __shfl_up(inc, 1, 64);
  *exc = lane == 0 ? 0.0 : e;
  return inc;
}

// Workgroup b walks the tiles of run b, [b R, min((b + 1) R, ntiles)): per tile the sum S of
// its samples (compute only); L[t] = the sum of the run's tiles before t, A[b] = the run's
// sum. red alternates per tile: one barrier per tile is enough. No occupancy bound: the usual
// expression stays under 64 VGPRs by itself (8 workgroups per CU: all 2048 runs resident at
// once on 256 CUs), a heavy one would spill under a bound.
extern "C" __global__ __launch_bounds__(256) void miint_expr_scan_tile_sums(
    double a, double h, double off, u64 i0, u64 n, unsigned ntiles, unsigned R,
    double* __restrict__ L, double* __restrict__ A) {
  __shared__ double red[2][4];
  const unsigned tb = blockIdx.x * R;
  const unsigned te = tb + R < ntiles ? tb + R : ntiles;
  double run = 0.0;
  unsigned par = 0;
  for (unsigned t = tb; t < te; ++t, par ^= 1u) {
    // four samples in flight, as miint_expr_partials has them (the loop is kept rolled: sixteen
    // at once take the registers of a second workgroup per SIMD, or spill)
    const u64 g = (u64)t * 4096ull + threadIdx.x * 16u;
    double idx = (double)(i0 + g) + off;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (g + 16 <= n) {
#pragma nounroll
      for (int k = 0; k < 16; k += 4) {
        a0 += miint_f(fma(idx, h, a));
        a1 += miint_f(fma(idx + 1.0, h, a));
        a2 += miint_f(fma(idx + 2.0, h, a));
        a3 += miint_f(fma(idx + 3.0, h, a));
        idx += 4.0;
      }
    } else {
#pragma nounroll
      for (int k = 0; k < 16; k += 4) {
        if (g + k < n) a0 += miint_f(fma(idx, h, a));
        if (g + k + 1 < n) a1 += miint_f(fma(idx + 1.0, h, a));
        if (g + k + 2 < n) a2 += miint_f(fma(idx + 2.0, h, a));
        if (g + k + 3 < n) a3 += miint_f(fma(idx + 3.0, h, a));
        idx += 4.0;
      }
    }
    double acc = (a0 + a1) + (a2 + a3);
    MIINT_BLOCK_SUM(acc, red[par]);
    if (threadIdx.x == 0) {
      L[t] = run;
      run += MIINT_RED(red[par]);
    }
  }
  if (threadIdx.x == 0) A[blockIdx.x] = run;
}

// One workgroup of 1024 threads over the nruns <= 2048 run sums, ceil(nruns / 1024)
// consecutive runs per thread: the thread's sum, one block scan (wave scans, then the lower
// waves' totals in order), then B[b] (exclusive) along the thread's runs. T[0] = the slice sum.
extern "C" __global__ __launch_bounds__(1024) void miint_expr_scan_tile_prefix(
    const double* __restrict__ A, unsigned nruns, double* __restrict__ B,
    double* __restrict__ T) {
  __shared__ double wt[16];
  const unsigned per = (nruns + 1023u) / 1024u;
  unsigned rb = threadIdx.x * per;
  if (rb > nruns) rb = nruns;
  unsigned re = rb + per;
  if (re > nruns) re = nruns;
  double s = 0.0;
  for (unsigned r = rb; r < re; ++r) s += A[r];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double exc;
  const double inc = miint_wave_scan(s, lane, &exc);
  if (lane == 63) wt[w] = inc;
  __syncthreads();
  double wb = 0.0;
  for (int q = 0; q < w; ++q) wb += wt[q];
  double run = wb + exc;
  for (unsigned r = rb; r < re; ++r) {
    B[r] = run;
    run += A[r];
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int q = 0; q < 16; ++q) tot += wt[q];
    T[0] = tot;
  }
}

// 16-byte chunk c of the tile lives at LDS chunk c ^ ((c >> 3) & 15): conflict-free for the
// ds_write_b128 of thread t (chunks 8t .. 8t+7) and for the ds_read_b128 of chunk k*256 + t
// (the swizzle of ts_write, trainscan.hip).
__device__ __forceinline__ int miint_swz(int c) { return c ^ ((c >> 3) & 15); }

// F = (((C + P[t]) + (wb + exc)) + run_k) * hs, P[t] = B[t / R] + L[t], for the selected
// samples. Sample i (global index) is selected when (i + 1) % every == 0 and goes to
// out[(i + 1) / every - i0 / every - 1]. The workgroups stride over `items` work items:
//   every == 1          an item is a tile; it goes through LDS so that consecutive lanes
//                       store consecutive 16-byte chunks (vec != 0: out is 16-byte aligned);
//                       the ragged last tile stores element-wise
//   1 < every < 4096    an item is a tile; predicated 8-byte stores; a (last) tile without
//                       a selected sample is passed over before anything is evaluated
//   every >= 4096       a tile holds at most one selected sample: an item is an output; its
//                       tile is evaluated up to that sample and one value is stored
extern "C" __global__ __launch_bounds__(256) void miint_expr_scan_write(
    double a, double h, double off, u64 i0, u64 n, u64 every, u64 items, unsigned R, int vec,
    const double* __restrict__ L, const double* __restrict__ B,
    const double* __restrict__ carry, double hs, double* __restrict__ out) {
  __shared__ double wt[4];
  __shared__ __attribute__((aligned(16))) double buf[4096];
  const u64 q0 = i0 / every;  // selected samples before the slice
  const double c0 = carry ? carry[0] : 0.0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (u64 item = blockIdx.x; item < items; item += gridDim.x) {
    u64 t = item, lim = n;
    if (every >= 4096ull) {
      const u64 gsel = (q0 + item + 1ull) * every - 1ull - i0;  // slice-local, < n
      t = gsel >> 12;
      lim = gsel + 1ull;
    }
    const u64 t0 = t * 4096ull;
    if (every > 1ull && every < 4096ull) {
      const u64 gfirst = ((i0 + t0) / every + 1ull) * every - 1ull - i0;  // first one >= t0
      if (gfirst >= n || gfirst >= t0 + 4096ull) continue;  // workgroup-uniform
    }
    const u64 g = t0 + threadIdx.x * 16u;
    double v[16];
    miint_items(a, h, off, i0, g, lim, v);
    double run = v[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
      run += v[k];
      v[k] = run;  // thread-serial inclusive scan
    }
    double exc;
    const double inc = miint_wave_scan(run, lane, &exc);
    if (lane == 63) wt[w] = inc;
    __syncthreads();
    double wb = 0.0;
    for (int q = 0; q < w; ++q) wb += wt[q];
    const double base = (c0 + (B[(unsigned)t / R] + L[t])) + (wb + exc);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (base + v[k]) * hs;

    if (every == 1ull) {
      // blocked (thread-contiguous) -> LDS -> striped stores
#pragma unroll
      for (int k = 0; k < 16; k += 2) {
        const int c = miint_swz((threadIdx.x * 16 + k) >> 1);
        *reinterpret_cast<f64x2*>(&buf[2 * c]) = f64x2{v[k], v[k + 1]};
      }
      __syncthreads();
      const bool wide = vec != 0 && t0 + 4096ull <= n;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = 2 * (k * 256 + (int)threadIdx.x);  // element pair index within the tile
        const f64x2 p = *reinterpret_cast<const f64x2*>(&buf[2 * miint_swz(e >> 1)]);
        if (wide) {
          *reinterpret_cast<f64x2*>(&out[t0 + e]) = p;
        } else {
          if (t0 + e < n) out[t0 + e] = p.x;
          if (t0 + e + 1 < n) out[t0 + e + 1] = p.y;
        }
      }
    } else if (every >= 4096ull) {
      // the item's one selected sample is lim - 1, its output position the item itself
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (g + k + 1 == lim) out[item] = v[k];
    } else if (g < lim) {
      // one 64-bit division per thread: q = selected samples of the slice before sample g,
      // r = (i0 + g) % every; sample g + k is selected when r + k + 1 reaches `every`
      u64 q = (i0 + g) / every;
      u64 r = (i0 + g) - q * every;
      q -= q0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (++r == every) {
          r = 0;
          if (g + k < lim) out[q] = v[k];
          ++q;
        }
      }
    }
    __syncthreads();  // wt and buf are written again by the next item
  }
}
)";
}

std::string expr_scan_compile(const std::string& expr) {
  return detail::rtc_compile_cached(expr_scan_source(expr), expr);
}

uint64_t expr_scan_outputs(uint64_t begin, uint64_t count, uint64_t every) {
  MIINT_CHECK(every >= 1, "expression scan: every must be >= 1 (got 0)");
  MIINT_CHECK(begin + count >= begin,
              "expression scan: begin " + std::to_string(begin) + " + count " +
                  std::to_string(count) + " wraps around 2^64");
  return (begin + count) / every - begin / every;
}

ScanShape expr_scan_shape(uint64_t count) {
  const uint64_t tiles = count / EXPR_SCAN_TILE + (count % EXPR_SCAN_TILE ? 1 : 0);
  MIINT_CHECK(tiles <= kExprScanMaxTiles,
              "expression scan: " + std::to_string(count) + " samples are " +
                  std::to_string(tiles) + " tiles of " + std::to_string(EXPR_SCAN_TILE) +
                  ", more than the " + std::to_string(kExprScanMaxTiles) +
                  " the tile prefix and its workspace are built for; slice the samples");
  ScanShape s;
  s.tiles = tiles;
  s.run = std::max<uint64_t>((tiles + kExprScanMaxRuns - 1) / kExprScanMaxRuns, 1);
  s.runs = (tiles + s.run - 1) / s.run;
  return s;
}

void expr_scan_check(uint64_t n, uint64_t begin, uint64_t count, uint64_t every,
                     uint64_t out_capacity) {
  const std::string slice = "samples [" + std::to_string(begin) + ", " + std::to_string(begin) +
                            " + " + std::to_string(count) + ")";
  MIINT_CHECK(begin + count >= begin, "expression scan: " + slice + " wrap around 2^64");
  MIINT_CHECK(detail::slice_in_range(n, begin, count),
              "expression scan: " + slice + " lie outside [0, n = " + std::to_string(n) + ")");
  MIINT_CHECK(every >= 1, "expression scan: every must be >= 1 (got 0)");
  (void)expr_scan_shape(count);
  const uint64_t outputs = expr_scan_outputs(begin, count, every);
  MIINT_CHECK(out_capacity >= outputs,
              "expression scan: the output buffer holds " + std::to_string(out_capacity) +
                  " values, " + slice + " with every = " + std::to_string(every) + " write " +
                  std::to_string(outputs));
}

ExprScan::ExprScan(const std::string& expr, int device)
    : expr_(expr), device_(device), stream_((set_device(device), Stream())),
      module_(expr_scan_compile(expr), device, stream_,
              {"miint_expr_scan_tile_sums", "miint_expr_scan_tile_prefix",
               "miint_expr_scan_write"}) {
  DeviceGuard g(device);
  runs_ = DeviceBuffer<double>(2 * kExprScanMaxRuns);  // A, then B
}

// L grows to the largest slice seen; the scalars to the largest world. Called with the
// stream idle (every run ends with a sync).
void ExprScan::reserve(uint64_t tiles, int world) {
  const size_t nt = std::max<uint64_t>(tiles, 1);
  if (local_.size() < nt) local_ = DeviceBuffer<double>(nt);
  const size_t w = static_cast<size_t>(std::max(world, 1));
  if (scalars_.size() < 2 + w) scalars_ = DeviceBuffer<double>(2 + w);
  if (host_.size() < w) host_ = PinnedBuffer<double>(w);
}

// K1 + K2: L, B and the slice sum T (scalars_[0]); T = 0 for an empty slice.
void ExprScan::enqueue_local(double a, double h, double off, uint64_t begin, uint64_t count,
                             hipStream_t s) {
  double* T = scalars_.get();
  if (count == 0) {
    MIINT_HIP(hipMemsetAsync(T, 0, sizeof(double), s));
    return;
  }
  const ScanShape shape = expr_scan_shape(count);
  const unsigned tiles = static_cast<unsigned>(shape.tiles), R = static_cast<unsigned>(shape.run);
  const unsigned runs = static_cast<unsigned>(shape.runs);
  double* A = runs_.get();
  double* B = A + kExprScanMaxRuns;
  module_.launch(kSums, runs, 1, kScanBlock, s, a, h, off, begin, count, tiles, R, local_.get(), A);
  module_.launch(kPrefix, 1, 1, kPrefixBlock, s, A, runs, B, T);
}

// K4: the workgroups stride over the tiles, or over the outputs once a tile holds at most
// one (every >= 4096).
void ExprScan::enqueue_write(double a, double h, double off, uint64_t begin, uint64_t count,
                             uint64_t every, const double* carry, double hs, double* out,
                             hipStream_t s) {
  const uint64_t outputs = expr_scan_outputs(begin, count, every);
  if (outputs == 0) return;
  const ScanShape shape = expr_scan_shape(count);
  const uint64_t items = every >= EXPR_SCAN_TILE ? outputs : shape.tiles;  // <= tiles
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(items, kExprScanMaxRuns));
  const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? 1 : 0;
  module_.launch(kWrite, grid, 1, kScanBlock, s, a, h, off, begin, count, every, items,
                 static_cast<unsigned>(shape.run), vec, local_.get(),
                 runs_.get() + kExprScanMaxRuns, carry, hs, out);
}

ExprScanResult ExprScan::run(double a, double b, uint64_t n, Rule rule, uint64_t begin,
                             uint64_t count, uint64_t every, double* out_device,
                             uint64_t out_capacity, double scale, const Comm* comm) {
  expr_scan_check(n, begin, count, every, out_capacity);
  const uint64_t outputs = expr_scan_outputs(begin, count, every);
  MIINT_CHECK(outputs == 0 || out_device != nullptr, "expression scan: no output buffer");
  const int world = comm ? comm->world() : 1;
  DeviceGuard g(device_);
  reserve(expr_scan_shape(count).tiles, world);
  const double h = (b - a) / static_cast<double>(n);
  const double hs = h * scale;
  const double off = rule_offset(rule);
  hipStream_t s = stream_.get();
  double* sc = scalars_.get();  // [0] T, [1] C, [2..) gathered
  e0_.record(s);
  enqueue_local(a, h, off, begin, count, s);
  const double* carry = nullptr;
  if (world > 1) {
    comm->allgather(sc, sc + 2, 1, s);
    launch_exclusive_carry(sc + 2, comm->rank(), sc + 1, s);
    carry = sc + 1;
  }
  enqueue_write(a, h, off, begin, count, every, carry, hs, out_device, s);
  e1_.record(s);
  MIINT_HIP(hipMemcpyAsync(host_.get(), world > 1 ? sc + 2 : sc, world * sizeof(double),
                           hipMemcpyDeviceToHost, s));
  stream_.sync();
  double tot = 0.0;
  for (int q = 0; q < world; ++q) tot += host_[q];  // rank order: the same on every rank
  ExprScanResult r;
  r.total = tot * hs;
  r.outputs = outputs;
  r.device_ms = Event::elapsed_ms(e0_, e1_);
  return r;
}

double ExprScan::time(double a, double b, uint64_t n, Rule rule, uint64_t begin, uint64_t count,
                      uint64_t every, double* out_device, uint64_t out_capacity, int iters) {
  MIINT_CHECK(iters >= 1, "bad expression scan timing request");
  expr_scan_check(n, begin, count, every, out_capacity);
  MIINT_CHECK(expr_scan_outputs(begin, count, every) == 0 || out_device != nullptr,
              "expression scan: no output buffer");
  DeviceGuard g(device_);
  reserve(expr_scan_shape(count).tiles, 1);
  const double h = (b - a) / static_cast<double>(n);
  const double off = rule_offset(rule);
  hipStream_t s = stream_.get();
  return detail::time_enqueues(stream_, e0_, e1_, iters, [&] {
    enqueue_local(a, h, off, begin, count, s);
    enqueue_write(a, h, off, begin, count, every, nullptr, h, out_device, s);
  });
}

}  // namespace miint
