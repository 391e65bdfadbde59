// Fused two-phase train-profile scan for gfx950: velocity samples -> running integral
// ("distance", 4main.c phase 1) -> running integral of that ("sum of sums", phase 2),
// written in ONE write-only pass over HBM.
//
// Reference (4main.c:76-221): fill 144 MB, local serial scan, gather all
// slices to rank 0, serial carry loop on rank 0, 144 MB broadcast; then the same again for
// phase 2. Its inputs are never data: every velocity sample is interp(profile, i*dt).
// That makes a reduce-then-scan free of input reads:
//
//   K1 ts_tile_sums   per 4096-sample tile t: S1 = sum_i v_i and S2 = sum_i (n_t - i) v_i
//                     (the sum of the tile's local inclusive prefix sums) — compute only
//   K2 ts_tile_prefix one workgroup: P1(t) = sum_{u<t} S1(u),
//                     Q(t) = sum_{u<t} [n_u P1(u) + S2(u)]   (DPP/LDS block scans), and the
//                     rank totals T1 = P1(end), T2 = Q(end)
//   (dt = 1/sps)      K1 + K2 as ONE launch, ts_tile_scan_closed: closed-form tile sums (one
//                     thread per tile), in-block scans, last-workgroup scan of the block
//                     aggregates; K4 composes block and in-block prefixes (6.8 us vs 22 us)
//   (multi-GPU)       allgather (T1, T2, count) per rank -> rank carries C1, C2 (K3)
//   K4 ts_write       per tile: recompute v, vel = C1 + P1(t) + local scan(v),
//                     pos = C2 + 4096 t C1 + Q(t) + local scan(vel); both transposed through
//                     LDS and stored with coalesced 16-byte stores
//
// HBM traffic: 2 x 8 bytes per sample, written once (vel, pos); nothing is read back.
// The 4main --parity fill windows (rank-private fills, 4main.c:76-86) are honoured: samples
// outside [win_lo, win_hi) are zero.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "miint/common.hpp"
#include "miint/handoff.hpp"
#include "miint/kernels.hpp"
#include "miint/trainscan.hpp"
#include "miint/wave_reduce.hpp"

namespace miint {
namespace {

constexpr int kB = 256;
constexpr int kItems = 16;
constexpr int kTile = kB * kItems;  // 4096 samples
constexpr int kMaxTable = 2048;
constexpr int kSpan = 64;  // table entries staged per tile (LDS)
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const double lds_f64;

// set_lds_poison: fill a tile's LDS window with NaN before staging (validation only)
__constant__ int g_lds_poison;

struct Sampler {
  const double* tab;  // LDS copy of table entries [s0, s0 + count), or the global table
  bool staged;        // tab points into LDS
  int s0, nseg;
  double dt;
  uint64_t i0, n, win_lo, win_hi;
  __device__ __forceinline__ double operator()(uint64_t g) const {  // g: slice-local index
    const uint64_t i = i0 + g;
    if (g >= n || i < win_lo || i >= win_hi) return 0.0;
    const double t = dt * static_cast<double>(i);
    int s = static_cast<int>(t);
    s = s < 0 ? 0 : (s >= nseg ? nseg - 1 : s);
    const double v0 = tab[s - s0];
    return fma(tab[s + 1 - s0] - v0, t - static_cast<double>(s), v0);
  }
  // The kItems consecutive samples of this thread, starting at slice-local index g.
  // Hot form (tile fully inside the slice and the fill window): 64-bit index math once per
  // thread, then per sample t = fma(k, dt, t_first), a 32-bit segment index and two
  // broadcast LDS reads — identical to operator() up to one rounding of t.
  // The hot form only runs on staged tiles and reads through an LDS-typed pointer: through
  // the generic pointer the compiler emits flat_load_dwordx4 pairs (8-byte aligned 16-byte
  // LDS reads: SQ_LDS_UNALIGNED_STALL 3.8e6 per pass) instead of ds_read2_b64.
  __device__ __forceinline__ void items(uint64_t g, bool plain, double (&v)[kItems]) const {
    if (!plain) {
#pragma unroll
      for (int k = 0; k < kItems; ++k) v[k] = (*this)(g + k);
      return;
    }
    lds_f64* lt = (lds_f64*)tab;
    const double tb = dt * static_cast<double>(i0 + g);
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const double t = fma(static_cast<double>(k), dt, tb);
      int s = static_cast<int>(t);
      s = s >= nseg ? nseg - 1 : s;
      const double v0 = lt[s - s0];
      v[k] = fma(lt[s + 1 - s0] - v0, t - static_cast<double>(s), v0);
    }
  }
  // Block-uniform: can every sample of tile [t0, t0 + kTile) take the hot form?
  __device__ __forceinline__ bool plain_tile(uint64_t t0) const {
    return staged && t0 + kTile <= n && i0 + t0 >= win_lo && i0 + t0 + kTile <= win_hi;
  }
};

__device__ __forceinline__ int seg_of(double t, int nseg) {
  int s = static_cast<int>(t);
  return s < 0 ? 0 : (s >= nseg ? nseg - 1 : s);
}

// Stage only the table entries this tile's samples touch: a 4096-sample tile at 1e4
// samples/s spans 0.41 s, i.e. 2-3 entries instead of the whole 14.4 KB table per
// workgroup (the full re-staging cost 63 MB of L2 reads per pass).
__device__ __forceinline__ Sampler make_sampler(const TrainScanKernelParams& p, double* tab,
                                                unsigned tile) {
  const int nseg = p.table_n - 1;
  const uint64_t t0 = static_cast<uint64_t>(tile) * kTile;
  const uint64_t last = (t0 + kTile < p.n ? t0 + kTile : p.n) - 1;
  const int s0 = seg_of(p.dt * static_cast<double>(p.i0 + t0), nseg);
  // Entries s0 .. s1: the last sample's segment, its right end, and one more. The hot form
  // forms t = fma(k, dt, t_first), which may round one ulp above dt * i; where dt * i sits
  // just below an integer that puts the sample in the NEXT segment with fraction 0, and the
  // read of that segment's right end must still land on a table value (weight 0), not on a
  // stale LDS word past the staged range (an Inf/NaN there would survive the 0 weight).
  const int s1 = min(seg_of(p.dt * static_cast<double>(p.i0 + last), nseg) + 2, nseg);
  if (s1 - s0 + 1 > kSpan)  // coarse sampling: read the (L2-resident) table directly
    return {p.table, false, 0, nseg, p.dt, p.i0, p.n, p.win_lo, p.win_hi};
  if (g_lds_poison) {  // validation: what the window does not stage reads as NaN
    for (int k = threadIdx.x; k < kSpan; k += kB) tab[k] = __builtin_nan("");
    __syncthreads();
  }
  for (int k = threadIdx.x; k <= s1 - s0; k += kB) tab[k] = p.table[s0 + k];
  __syncthreads();
  return {tab, true, s0, nseg, p.dt, p.i0, p.n, p.win_lo, p.win_hi};
}

// ---------------------------------------------------------------------------- K1
__global__ __launch_bounds__(kB) void ts_tile_sums(TrainScanKernelParams p, f64x2* sums) {
  __shared__ double tab[kSpan];
  __shared__ double red1[kB / kWave], red2[kB / kWave];
  const Sampler f = make_sampler(p, tab, blockIdx.x);
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  const uint64_t nt = p.n - t0 < kTile ? p.n - t0 : kTile;
  double v[kItems];
  f.items(t0 + threadIdx.x * kItems, f.plain_tile(t0), v);
  const double w0 = static_cast<double>(static_cast<int64_t>(nt) - threadIdx.x * kItems);
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    s1 += v[k];
    s2 = fma(w0 - k, v[k], s2);  // sample i is counted n_t - i times in the tile's prefixes
  }
  s1 = block_sum<kB>(s1, red1);
  s2 = block_sum<kB>(s2, red2);
  if (threadIdx.x == 0) sums[blockIdx.x] = f64x2{s1, s2};
}

// ---------------------------------------------------------------------------- K2
// One workgroup, a contiguous run of tiles per thread: serial within the thread, then two
// block scans in total (S1 -> P1, then q = n_t P1 + S2 -> Q). The earlier form scanned
// chunks of 1024 tiles with two block scans each (7.8 us for 4395 tiles).
constexpr int kPB = 1024;
__global__ __launch_bounds__(kPB) void ts_tile_prefix(const f64x2* sums, uint32_t ntiles,
                                                      uint64_t n, f64x2* prefix, double* totals) {
  __shared__ double red[kPB / kWave];
  const uint32_t per = (ntiles + kPB - 1) / kPB;
  const uint32_t tb = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles;
  const uint32_t te = tb + per < ntiles ? tb + per : ntiles;
  auto count = [&](uint32_t t) {
    const uint64_t t0 = static_cast<uint64_t>(t) * kTile;
    return static_cast<double>(n - t0 < kTile ? n - t0 : kTile);
  };
  double a = 0.0;
  for (uint32_t t = tb; t < te; ++t) a += sums[t].x;
  double tot1;
  const double base1 = block_inclusive_scan<kPB>(a, red, &tot1) - a;
  __syncthreads();
  double q = 0.0, p1 = base1;
  for (uint32_t t = tb; t < te; ++t) {
    const f64x2 st = sums[t];
    q += fma(count(t), p1, st.y);
    p1 += st.x;
  }
  double tot2;
  const double base2 = block_inclusive_scan<kPB>(q, red, &tot2) - q;
  double run_p = base1, run_q = base2;
  for (uint32_t t = tb; t < te; ++t) {
    const f64x2 st = sums[t];
    prefix[t] = f64x2{run_p, run_q};
    run_q += fma(count(t), run_p, st.y);
    run_p += st.x;
  }
  if (threadIdx.x == 0) {
    totals[0] = tot1;  // T1: slice sum of v
    totals[1] = tot2;  // T2: slice sum of the local running integral
  }
}

// ---------------------------------------------------------------------------- K1, closed form
// When dt = 1/sps for an integer sps, sample i lies in segment s = min(i / sps, nseg - 1) at
// fr = (i - s sps) dt, so a tile's samples are a few runs of an arithmetic sequence and its
// sums have closed forms: with j = i - s sps over [ja, jb), m = jb - ja, v = v0 + c j
// (c = (v1 - v0) dt) and weight n_t - l = W0 - j,
//   S1 += m v0 + c sum(j),   S2 += W0 m v0 + (W0 c - v0) sum(j) - c sum(j^2).
// One thread per tile instead of a workgroup re-sampling its 4096 points (14.5 us for 18e6
// samples). The samples themselves are computed and written by K4 only; the closed form
// differs from their rounded sum by ~1e-16 relative.
__device__ __forceinline__ uint64_t div_sps(uint64_t i, uint64_t sps, double inv) {
  uint64_t q = static_cast<uint64_t>(static_cast<double>(i) * inv);  // exact to +-1
  if (q * sps > i) --q;
  else if ((q + 1) * sps <= i) ++q;
  return q;
}

__device__ __forceinline__ f64x2 tile_sums_closed(const TrainScanKernelParams& p, uint64_t sps,
                                                  double inv_sps, uint64_t t) {
  const int64_t nseg = p.table_n - 1;
  const uint64_t g0 = t * kTile;
  const uint64_t g1 = g0 + kTile < p.n ? g0 + kTile : p.n;
  const uint64_t it0 = p.i0 + g0;  // global index of the tile's first sample
  uint64_t ia = it0 > p.win_lo ? it0 : p.win_lo;
  const uint64_t ib = p.i0 + g1 < p.win_hi ? p.i0 + g1 : p.win_hi;
  double s1 = 0.0, s2 = 0.0;
  while (ia < ib) {
    int64_t sg = static_cast<int64_t>(div_sps(ia, sps, inv_sps));
    if (sg > nseg - 1) sg = nseg - 1;
    const uint64_t base = static_cast<uint64_t>(sg) * sps;
    const uint64_t end = (sg == nseg - 1 || base + sps > ib) ? ib : base + sps;
    const double ja = static_cast<double>(ia - base), jb = static_cast<double>(end - base);
    const double m = jb - ja;
    const double sj = 0.5 * m * (ja + jb - 1.0);
    // sum_{ja <= j < jb} j^2 via (x-1) x (2x-1) / 6 (exact integers below 2^53)
    auto sq = [](double x) { return (x - 1.0) * x * (2.0 * x - 1.0); };
    const double sj2 = (sq(jb) - sq(ja)) * (1.0 / 6.0);
    const double v0 = p.table[sg];
    const double c = (p.table[sg + 1] - v0) * p.dt;
    const double w0 = static_cast<double>(static_cast<int64_t>(g1 - g0) +
                                          static_cast<int64_t>(it0) - static_cast<int64_t>(base));
    s1 += fma(c, sj, m * v0);
    s2 += fma(fma(w0, c, -v0), sj, w0 * m * v0) - c * sj2;
    ia = end;
  }
  return f64x2{s1, s2};
}

// K1 + K2 in one launch: thread t computes tile t's closed-form sums; the block scans its
// 256 tiles (local[t] = in-block exclusive {P1, Q}) and publishes its aggregate {A, B, N}
// (sc1 stores, drain, agent-scope ticket); the block drawing the last ticket acquires and
// scans the block aggregates into block prefixes {PB, QB} and the slice totals. K4 composes
// P1(t) = PB + P1l(t), Q(t) = QB + (t mod 256) 4096 PB + Ql(t). The former one-workgroup
// K2 took 7.8-8.7 us of serial memory latency for 4395 tiles.
struct ClosedScan {
  f64x2* local;      // per tile, in-block exclusive {P1, Q}
  f64x2* blockpre;   // per block, exclusive {PB, QB}
  double* agg;       // per block {A, B, N} (stride 4 doubles)
  unsigned* ticket;
  unsigned* timeout;  // raised by a block-aggregate slot wait that gave up (ticket + 1)
};

// kHandoff = false (one GPU, <= kMaxFoldBlocks blocks): stop after the per-block aggregates;
// ts_write folds the few aggregates before its own block itself, so this launch ends without
// the ticket round trips and the last workgroup's serial block scan.
constexpr uint32_t kMaxFoldBlocks = 64;  // blocks of kB tiles: 64 x 256 x 4096 = 67M samples

template <bool kHandoff>
__global__ __launch_bounds__(kB) void ts_tile_scan_closed(TrainScanKernelParams p, uint64_t sps,
                                                          uint32_t ntiles, ClosedScan cs,
                                                          double* totals) {
  __shared__ double red[kB / kWave];
  __shared__ int is_last;
  const uint32_t t = blockIdx.x * kB + threadIdx.x;
  const bool valid = t < ntiles;
  const f64x2 st = valid ? tile_sums_closed(p, sps, 1.0 / static_cast<double>(sps), t)
                         : f64x2{0.0, 0.0};
  const uint64_t t0 = static_cast<uint64_t>(t) * kTile;
  const double cnt = valid ? static_cast<double>(p.n - t0 < kTile ? p.n - t0 : kTile) : 0.0;
  double A, B, N;
  const double p1 = block_inclusive_scan<kB>(st.x, red, &A) - st.x;
  __syncthreads();
  const double q = fma(cnt, p1, st.y);
  const double ql = block_inclusive_scan<kB>(q, red, &B) - q;
  __syncthreads();
  block_inclusive_scan<kB>(cnt, red, &N);
  if (valid) cs.local[t] = f64x2{p1, ql};
  if constexpr (!kHandoff) {
    if (threadIdx.x == 0) {  // read by the next launch: the kernel boundary orders it
      double* g = cs.agg + 4 * blockIdx.x;
      g[0] = A;
      g[1] = B;
      g[2] = N;
    }
    return;
  }
  if (threadIdx.x == 0) {  // write-once slots (handoff.hpp), filled unset by the launcher
    double* g = cs.agg + 4 * blockIdx.x;
    slot_store(g, A);
    slot_store(g + 1, B);
    slot_store(g + 2, N);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // latency only
    const unsigned prev =
        __hip_atomic_fetch_add(cs.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    is_last = (prev == gridDim.x - 1);
  }
  __syncthreads();
  if (!is_last) return;
  // exclusive scan over the block aggregates, kB at a time (affine: Q += N PB + B)
  double cp = 0.0, cq = 0.0;
  for (uint32_t b0 = 0; b0 < gridDim.x; b0 += kB) {
    const uint32_t b = b0 + threadIdx.x;
    const bool vb = b < gridDim.x;
    const double* g = cs.agg + 4 * b;
    const double a = vb ? slot_wait(g, slot_load(g), cs.timeout) : 0.0;
    const double bb = vb ? slot_wait(g + 1, slot_load(g + 1), cs.timeout) : 0.0;
    const double nb = vb ? slot_wait(g + 2, slot_load(g + 2), cs.timeout) : 0.0;
    double ta, tq;
    const double pb = cp + (block_inclusive_scan<kB>(a, red, &ta) - a);
    __syncthreads();
    const double qq = fma(nb, pb, bb);
    const double qb = cq + (block_inclusive_scan<kB>(qq, red, &tq) - qq);
    __syncthreads();
    if (vb) cs.blockpre[b] = f64x2{pb, qb};
    cp += ta;
    cq += tq;
  }
  if (threadIdx.x == 0) {
    totals[0] = cp;  // T1: slice sum of v
    totals[1] = cq;  // T2: slice sum of the local running integral
    __hip_atomic_store(cs.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
  }
}

ClosedScan closed_carve(void* ws, uint64_t nt) {
  const uint64_t nb = (nt + kB - 1) / kB;
  ClosedScan cs;
  cs.local = static_cast<f64x2*>(ws);
  cs.blockpre = cs.local + nt;
  cs.agg = reinterpret_cast<double*>(cs.blockpre + nb);
  cs.ticket = reinterpret_cast<unsigned*>(cs.agg + 4 * nb);
  cs.timeout = cs.ticket + 1;
  return cs;
}

bool closed_form_sps(double dt, uint64_t* sps) {
  const double r = 1.0 / dt;
  const double k = std::nearbyint(r);
  if (!(k >= 1.0 && std::fabs(r - k) <= 1e-9 * r)) return false;
  *sps = static_cast<uint64_t>(k);
  return true;
}

// ---------------------------------------------------------------------------- K3
// gathered: world x {T1, T2, count}. carries = {C1, C2} for `rank` (fixed order everywhere).
__global__ void ts_rank_carry(const double* gathered, int rank, double* carries) {
  double c1 = 0.0, c2 = 0.0;
  for (int q = 0; q < rank; ++q) {
    const double t1 = gathered[3 * q], t2 = gathered[3 * q + 1], cnt = gathered[3 * q + 2];
    c2 += fma(cnt, c1, t2);  // rank q's position total = count_q * C1(q) + T2(q)
    c1 += t1;
  }
  carries[0] = c1;
  carries[1] = c2;
}

// ---------------------------------------------------------------------------- K4
// 16-byte chunk c of the tile lives at LDS chunk c ^ ((c >> 3) & 15): conflict-free for
// both sides of the transpose (MI355X_MICROARCH.md §LDS) — the ds_write_b128 of thread t
// (chunks 8t..8t+7, 8 contiguous lanes per group, banks (a/4) mod 32) and the ds_read_b128
// of chunk k*256 + t (4 non-contiguous 16-lane groups, banks (a/4) mod 64). A +16 B per
// 128 B padding was conflict-free only for the writes (1.1e6 conflict cycles per pass).
__device__ __forceinline__ int swz(int c) { return c ^ ((c >> 3) & 15); }

__device__ __forceinline__ void store_tile(double* buf, const double (&v)[kItems], double* out,
                                           uint64_t t0, uint64_t n) {
  // blocked (thread-contiguous) -> LDS -> striped 16-byte stores
#pragma unroll
  for (int k = 0; k < kItems; k += 2) {
    const int c = swz((threadIdx.x * kItems + k) >> 1);
    *reinterpret_cast<f64x2*>(&buf[2 * c]) = f64x2{v[k], v[k + 1]};
  }
  __syncthreads();
  const bool full = t0 + kTile <= n;
#pragma unroll
  for (int k = 0; k < kItems / 2; ++k) {
    const int e = 2 * (k * kB + threadIdx.x);  // element pair index within the tile
    const f64x2 w = *reinterpret_cast<const f64x2*>(&buf[2 * swz(e >> 1)]);
    if (full) {
      *reinterpret_cast<f64x2*>(&out[t0 + e]) = w;
    } else {
      if (t0 + e < n) out[t0 + e] = w.x;
      if (t0 + e + 1 < n) out[t0 + e + 1] = w.y;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kB) void ts_write(TrainScanKernelParams p, const f64x2* prefix,
                                               const f64x2* blockpre, const double* fold_agg,
                                               const double* carries, double* vel,
                                               double* pos) {
  __shared__ double tab[kSpan];
  __shared__ double red[kB / kWave];
  __shared__ __attribute__((aligned(16))) double buf[kTile];
  const Sampler f = make_sampler(p, tab, blockIdx.x);
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  f64x2 pr = prefix[blockIdx.x];
  if (fold_agg) {  // fold mode: this tile's block prefix from the aggregates before it
    __shared__ double agg[3 * kMaxFoldBlocks];
    __shared__ double bpf[2];
    const uint32_t b = blockIdx.x / kB;
    if (threadIdx.x < b) {
      agg[3 * threadIdx.x] = fold_agg[4 * threadIdx.x];
      agg[3 * threadIdx.x + 1] = fold_agg[4 * threadIdx.x + 1];
      agg[3 * threadIdx.x + 2] = fold_agg[4 * threadIdx.x + 2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // same affine fold as ts_rank_carry: Q += N PB + B, PB += A
      double pb = 0.0, qb = 0.0;
      for (uint32_t i = 0; i < b; ++i) {
        qb += fma(agg[3 * i + 2], pb, agg[3 * i + 1]);
        pb += agg[3 * i];
      }
      bpf[0] = pb;
      bpf[1] = qb;
    }
    __syncthreads();
    const double before = static_cast<double>(blockIdx.x % kB) * kTile;
    pr = f64x2{bpf[0] + pr.x, fma(before, bpf[0], bpf[1]) + pr.y};
  } else if (blockpre) {  // closed-form path: tile prefix = block prefix (+) in-block prefix
    const f64x2 bp = blockpre[blockIdx.x / kB];
    const double before = static_cast<double>(blockIdx.x % kB) * kTile;
    pr = f64x2{bp.x + pr.x, fma(before, bp.x, bp.y) + pr.y};
  }
  const double c1 = carries ? carries[0] : 0.0;
  const double c2 = carries ? carries[1] : 0.0;
  double v[kItems];
  f.items(t0 + threadIdx.x * kItems, f.plain_tile(t0), v);
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    run += v[k];
    v[k] = run;  // thread-local inclusive scan of the samples
  }
  double tot;
  const double ex1 = block_inclusive_scan<kB>(run, red, &tot) - run;
  const double base1 = (c1 + pr.x) + ex1;
#pragma unroll
  for (int k = 0; k < kItems; ++k) v[k] += base1;  // velocity integral ("distance")
  if (vel) store_tile(buf, v, vel, t0, p.n);
  __syncthreads();
  run = 0.0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    run += v[k];
    v[k] = run;
  }
  const double ex2 = block_inclusive_scan<kB>(run, red, &tot) - run;
  const double base2 = (c2 + fma(static_cast<double>(t0), c1, pr.y)) + ex2;
#pragma unroll
  for (int k = 0; k < kItems; ++k) v[k] += base2;  // running integral of the above
  if (pos) store_tile(buf, v, pos, t0, p.n);
}

// ---------------------------------------------------------------------------- one pass
// Single GPU: K1 + K2 + K4 in ONE pass with a decoupled look-back (as scan.hip) over the
// two-component tile state (A, B) = (sum v, sum of the tile's local running integral).
// Concatenation is affine — (A1,B1) then (A2,B2) = (A1+A2, B1 + B2 + n2 A1) — but every
// predecessor of a tile is a full 4096-sample tile, so the exclusive state of tile t is a
// plain sum over predecessors j of (A_j, B_j + 4096 (t-1-j) A_j), and over the nearest
// predecessor s that published its inclusive state (P_s, Q_s): (P_s, Q_s + 4096 (t-1-s) P_s).
// Commutative terms: the wave sums them with DPP exactly like the 1-component look-back.
// Samples are generated once and HBM sees only the 16 B/sample of vel + pos stores.
// Tile ids come from an atomic counter (forward progress under any dispatch order). The tile
// states are write-once slots (handoff.hpp): {A, B} aggregate and {P, Q} prefix pairs, each
// component its own slot; a lane that sees a pair's first component set waits for the
// second. Spins are bounded (NaN + the timeout word). The look-back sums whatever mix of
// aggregates and prefixes it finds, so the last bits may differ run to run; the 3-kernel
// path (ScanAlgo::kFused) is the bitwise-deterministic one.
constexpr size_t kOpHeader = 64;  // counter @0, timeout @4

struct OnePassState {
  unsigned* counter;
  unsigned* timeout;
  double* agg;      // per tile {A, B} (slots)
  double* pref;     // per tile inclusive {P, Q} (slots)
};

__device__ __forceinline__ void op_publish(double* slot, unsigned tile, double x, double y) {
  slot_store(slot + 2 * tile, x);
  slot_store(slot + 2 * tile + 1, y);
}

// Wave 0: exclusive {P, Q} of `tile` (lanes examine tile-1-lane, 64 at a time).
__device__ f64x2 op_look_back(const OnePassState& st, unsigned tile) {
  const int lane = threadIdx.x & 63;
  double P = 0.0, Q = 0.0;
  long base = static_cast<long>(tile) - 1;
  for (;;) {
    const long j = base - lane;
    bool is_pref = true;  // lanes past the front act as "prefix 0"
    double a = 0.0, b = 0.0;
    if (j >= 0) {
      unsigned spins = 0;
      const double* src = nullptr;
      for (;;) {
        a = slot_load(st.pref + 2 * j);
        if (!slot_unset(a)) {
          src = st.pref + 2 * j;
          break;
        }
        a = slot_load(st.agg + 2 * j);
        if (!slot_unset(a)) {
          src = st.agg + 2 * j;
          is_pref = false;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        if (++spins > kSlotSpinLimit) {
          __hip_atomic_store(st.timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          a = __builtin_nan("");
          break;
        }
      }
      b = src ? slot_wait(src + 1, slot_load(src + 1), st.timeout) : a;
    }
    const unsigned long long pm = __ballot(is_pref);
    const int stop = pm ? __builtin_ctzll(pm) : 64;
    const double gap = static_cast<double>(kTile) * static_cast<double>(static_cast<long>(tile) - 1 - j);
    const bool use = lane <= stop && j >= 0;
    P += wave_sum(use ? a : 0.0);
    Q += wave_sum(use ? fma(gap, a, b) : 0.0);
    if (pm) break;
    base -= 64;
  }
  return f64x2{P, Q};
}

__global__ __launch_bounds__(kB) void ts_onepass(TrainScanKernelParams p, OnePassState st,
                                                 unsigned ntiles, double* vel, double* pos,
                                                 double* totals) {
  __shared__ double tab[kSpan];
  __shared__ double red[kB / kWave];
  __shared__ __attribute__((aligned(16))) double buf[kTile];
  __shared__ unsigned tile_sh;
  __shared__ double pre_sh[2];
  if (threadIdx.x == 0)
    tile_sh = __hip_atomic_fetch_add(st.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const unsigned tile = tile_sh;
  const Sampler f = make_sampler(p, tab, tile);
  const uint64_t t0 = static_cast<uint64_t>(tile) * kTile;
  const double nt = static_cast<double>(p.n - t0 < kTile ? p.n - t0 : kTile);
  double v[kItems], w[kItems];
  f.items(t0 + threadIdx.x * kItems, f.plain_tile(t0), v);
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    run += v[k];
    v[k] = run;
  }
  double A;
  const double ex1 = block_inclusive_scan<kB>(run, red, &A) - run;
  __syncthreads();  // red is reused
  run = 0.0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    v[k] += ex1;  // tile-local running integral of v
    run += v[k];
    w[k] = run;
  }
  double Bt;
  const double ex2 = block_inclusive_scan<kB>(run, red, &Bt) - run;
  // a partial (last) tile's padding holds v = 0, so each padded slot carries the running
  // total A into Bt: only the first nt slots belong to the slice
  Bt = fma(nt - static_cast<double>(kTile), A, Bt);
#pragma unroll
  for (int k = 0; k < kItems; ++k) w[k] += ex2;  // tile-local running integral of that
  if (threadIdx.x < kWave) {
    f64x2 ex = {0.0, 0.0};
    if (tile > 0) {
      if (threadIdx.x == 0) op_publish(st.agg, tile, A, Bt);
      ex = op_look_back(st, tile);
    }
    if (threadIdx.x == 0) {
      const double pi = ex.x + A, qi = fma(nt, ex.x, ex.y + Bt);
      op_publish(st.pref, tile, pi, qi);
      pre_sh[0] = ex.x;
      pre_sh[1] = ex.y;
      if (tile + 1 == ntiles) {
        totals[0] = pi;  // T1, T2 of this slice
        totals[1] = qi;
      }
    }
  }
  __syncthreads();
  const double P = pre_sh[0], Q = pre_sh[1];
#pragma unroll
  for (int k = 0; k < kItems; ++k) v[k] += P;  // velocity integral ("distance")
  store_tile(buf, v, vel, t0, p.n);
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const double cnt = static_cast<double>(threadIdx.x * kItems + k + 1);
    w[k] = Q + fma(cnt, P, w[k]);  // running integral of the above
  }
  store_tile(buf, w, pos, t0, p.n);
}

OnePassState op_carve(void* ws, uint64_t nt) {
  char* p = static_cast<char*>(ws);
  OnePassState st;
  st.counter = reinterpret_cast<unsigned*>(p);
  st.timeout = reinterpret_cast<unsigned*>(p + 4);
  st.agg = reinterpret_cast<double*>(p + kOpHeader);
  st.pref = st.agg + 2 * nt;
  return st;
}

// --parity distance, bit-exact with 4main.c: the reference's rank fills its
// private InterpProfile over its fill window (4main.c:76-86, faccel at :262-269: truncating
// index, separate multiply and add) and scans its element slice with ONE sequential fp64
// running sum (4main.c:101-107 / 118-122). Any parallel scan rounds differently, and the
// printed 6th decimal sees it (P = 16: 117642.707174 vs .707175), so the printed element is
// reproduced with the reference's own dependency chain: the workgroup evaluates 256 samples
// per round in parallel, lane 0 adds them in index order. out[0] = running sum at the slice's
// last element, out[1] = running sum at global element `want` (0 if outside the slice).
// Parity mode only (one workgroup, ~n x add latency); the rank carries are added on the host
// in the reference's order (trainscan.cpp).
__global__ __launch_bounds__(256) void ts_parity_serial(TrainScanKernelParams p, uint64_t want,
                                                        double* out) {
#pragma clang fp contract(off)
  __shared__ double vals[256];
  double local = 0.0, at = 0.0;
  for (uint64_t base = 0; base < p.n; base += 256) {
    const uint64_t j = base + threadIdx.x;
    double v = 0.0;
    if (j < p.n) {
      const uint64_t i = p.i0 + j;
      if (i >= p.win_lo && i < p.win_hi) {
        const double t = 0.0 + p.dt * static_cast<double>(i);
        // the reference's truncating index; its windows never reach the last entry, and the
        // clamp (a no-op there) keeps any other window inside the table
        const int k = min(static_cast<int>(t), p.table_n - 2);
        const double delta = t - static_cast<double>(k);
        const double prod = (p.table[k + 1] - p.table[k]) * delta;
        v = p.table[k] + prod;
      }
    }
    vals[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint64_t m = p.n - base < 256 ? p.n - base : 256;
      const uint64_t hit = want - p.i0 - base;  // wraps (never < m) when want is elsewhere
      for (uint64_t q = 0; q < m; ++q) {
        local = local + vals[q];
        if (q == hit) at = local;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = local;
    out[1] = at;
  }
}

}  // namespace

void set_lds_poison_trainscan(bool on) {
  const int v = on ? 1 : 0;
  MIINT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_lds_poison), &v, sizeof(v)));
}

size_t trainscan_workspace_bytes(uint64_t n) {
  const uint64_t nt = (n + kTile - 1) / kTile;
  // 3-kernel path: {sums, prefix} f64x2 per tile + per-block {prefix, aggregates, ticket};
  // one-pass: header + {agg, pref} slot pairs per tile. The one-pass layout is the larger.
  return kOpHeader + 2 * nt * sizeof(f64x2);
}

void launch_trainscan_onepass(const TrainScanKernelParams& p, void* ws, double* vel, double* pos,
                              double* totals, hipStream_t s) {
  MIINT_CHECK(p.n >= 1, "empty slice");
  MIINT_CHECK(p.table_n >= 2 && p.table_n <= kMaxTable, "table size must be in [2, 2048]");
  MIINT_CHECK(vel && pos && totals, "one-pass scan writes vel, pos and totals");
  MIINT_CHECK((reinterpret_cast<uintptr_t>(vel) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(pos) & 15) == 0,
              "trainscan outputs need 16-B alignment");
  const uint64_t nt = (p.n + kTile - 1) / kTile;
  MIINT_CHECK(nt < (1u << 31), "slice too large");
  const OnePassState st = op_carve(ws, nt);
  MIINT_HIP(hipMemsetAsync(ws, 0, kOpHeader, s));
  fill_unset_slots(st.agg, 4 * nt, s);
  ts_onepass<<<static_cast<unsigned>(nt), kB, 0, s>>>(p, st, static_cast<unsigned>(nt), vel, pos,
                                                       totals);
  MIINT_HIP(hipGetLastError());
}

unsigned trainscan_onepass_timeout(const void* ws, hipStream_t s) {
  unsigned v = 0;
  MIINT_HIP(hipMemcpyAsync(&v, static_cast<const char*>(ws) + 4, sizeof(v), hipMemcpyDeviceToHost,
                           s));
  MIINT_HIP(hipStreamSynchronize(s));
  return v;
}

unsigned trainscan_local_timeout(const TrainScanKernelParams& p, const void* ws,
                                 hipStream_t s) {
  uint64_t sps = 0;
  if (!closed_form_sps(p.dt, &sps)) return 0;  // the 3-kernel path hands nothing over
  const ClosedScan cs = closed_carve(const_cast<void*>(ws), (p.n + kTile - 1) / kTile);
  unsigned v = 0;
  MIINT_HIP(hipMemcpyAsync(&v, cs.timeout, sizeof(v), hipMemcpyDeviceToHost, s));
  MIINT_HIP(hipStreamSynchronize(s));
  return v;
}

static bool use_fold(const TrainScanKernelParams& p, bool fold) {
  uint64_t sps = 0;
  const uint64_t nt = (p.n + kTile - 1) / kTile;
  return fold && closed_form_sps(p.dt, &sps) && (nt + kB - 1) / kB <= kMaxFoldBlocks;
}

bool trainscan_fold_applies(const TrainScanKernelParams& p) { return use_fold(p, true); }

void launch_trainscan_local(const TrainScanKernelParams& p, void* ws, double* totals,
                            hipStream_t s, bool fold) {
  MIINT_CHECK(p.n >= 1, "empty slice");
  MIINT_CHECK(p.table_n >= 2 && p.table_n <= kMaxTable, "table size must be in [2, 2048]");
  const uint64_t nt = (p.n + kTile - 1) / kTile;
  MIINT_CHECK(nt < (1u << 31), "slice too large");
  uint64_t sps = 0;
  if (closed_form_sps(p.dt, &sps)) {  // dt = 1/sps: closed-form tile sums, one launch
    // the ticket is zero from allocation (workspace contract) and re-armed by the kernel
    const ClosedScan cs = closed_carve(ws, nt);
    if (use_fold(p, fold))
      ts_tile_scan_closed<false><<<static_cast<unsigned>((nt + kB - 1) / kB), kB, 0, s>>>(
          p, sps, static_cast<uint32_t>(nt), cs, totals);
    else {
      // the block-aggregate hand-off: write-once slots, armed here (a few doubles per block)
      fill_unset_slots(cs.agg, 4 * ((nt + kB - 1) / kB), s);
      ts_tile_scan_closed<true><<<static_cast<unsigned>((nt + kB - 1) / kB), kB, 0, s>>>(
          p, sps, static_cast<uint32_t>(nt), cs, totals);
    }
    MIINT_HIP(hipGetLastError());
    return;
  }
  f64x2* sums = static_cast<f64x2*>(ws);
  f64x2* prefix = sums + nt;
  ts_tile_sums<<<static_cast<unsigned>(nt), kB, 0, s>>>(p, sums);
  MIINT_HIP(hipGetLastError());
  ts_tile_prefix<<<1, kPB, 0, s>>>(sums, static_cast<uint32_t>(nt), p.n, prefix, totals);
  MIINT_HIP(hipGetLastError());
}

void launch_trainscan_rank_carry(const double* gathered, int rank, double* carries,
                                 hipStream_t s) {
  ts_rank_carry<<<1, 1, 0, s>>>(gathered, rank, carries);
  MIINT_HIP(hipGetLastError());
}

void launch_trainscan_write(const TrainScanKernelParams& p, const void* ws, const double* carries,
                            double* vel, double* pos, hipStream_t s, bool fold) {
  MIINT_CHECK((reinterpret_cast<uintptr_t>(vel) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(pos) & 15) == 0,
              "trainscan outputs need 16-B alignment");
  const uint64_t nt = (p.n + kTile - 1) / kTile;
  uint64_t sps = 0;
  if (closed_form_sps(p.dt, &sps)) {  // layout of launch_trainscan_local's closed-form path
    const ClosedScan cs = closed_carve(const_cast<void*>(ws), nt);
    const bool f = use_fold(p, fold);
    MIINT_CHECK(!f || carries == nullptr, "fold mode is single-GPU (no rank carries)");
    ts_write<<<static_cast<unsigned>(nt), kB, 0, s>>>(p, cs.local, f ? nullptr : cs.blockpre,
                                                      f ? cs.agg : nullptr, carries, vel, pos);
  } else {
    const f64x2* prefix = static_cast<const f64x2*>(ws) + nt;
    ts_write<<<static_cast<unsigned>(nt), kB, 0, s>>>(p, prefix, nullptr, nullptr, carries, vel,
                                                      pos);
  }
  MIINT_HIP(hipGetLastError());
}

void launch_trainscan_parity_serial(const TrainScanKernelParams& p, uint64_t want, double* out,
                                    hipStream_t s) {
  MIINT_CHECK(p.n >= 1, "parity serial scan needs a non-empty slice");
  // every sample it may evaluate reads table[k + 1] with k = (int)(i * dt): i < win_hi and
  // i < i0 + n, so the largest time must stay inside the table
  const uint64_t hi = std::min<uint64_t>(p.win_hi, p.i0 + p.n);
  MIINT_CHECK(hi == 0 || static_cast<double>(hi - 1) * p.dt < static_cast<double>(p.table_n - 1),
              "parity serial scan: samples beyond the table");
  ts_parity_serial<<<1, 256, 0, s>>>(p, want, out);
  MIINT_HIP(hipGetLastError());
}

}  // namespace miint
