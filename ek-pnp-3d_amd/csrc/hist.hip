// hist.hip — histograms and joint histograms of the fields per z plane, the range of a value per plane, and a time series of
// histograms (include/ekpnp.h: ekpnp_hist_bin, ekpnp_hist_spec_check, ekpnp_hist_planes, ekpnp_value_range, ekpnp_hist_*; no
// reference counterpart).
//
// A count is an integer: it does not depend on the order of the additions, so the counts of a plane are the same in a two-buffer,
// an in-place, a slab context and any group whatever the grid - nothing here needs a fixed order, and nothing is a float atomic.
//   hist_index               THE definition, host and device alike (every operation rounded once: the object is built with
//                            -ffp-contract=off, csrc/Makefile PINNED); `scale` is formed once on the host and handed to the kernel
//   k_hist_partials<2D,QA,QB>  grid (workgroups per plane, planes), 256 threads.  A workgroup takes `chunk` consecutive nodes of ONE
//                            plane, tile after tile; a tile is 16 loads per thread, all in flight before the first is used (16, 8
//                            or 4 per array for one, two or three/four arrays), 16 B each where every plane base is 16-byte aligned
//                            (a wave-uniform branch: an odd plane of an odd z, a caller-bound array at an odd double take the 8 B
//                            path).  It reads only the arrays the spec names: 8 B per node for a field, 16 B for q = c - cn, at
//                            most 32 B for q against q.  cells + 1 uint32 counters in LDS (dynamic, (cells + 1) * 4 B: 520 B for
//                            128 bins, 17.4 KB for 64 x 64, 49 KB for the largest spec 1 x 4096), zeroed, added to with no-return
//                            LDS integer atomics, then stored as the workgroup's partial counts with plain vector stores.
//   k_hist_finish            a thread per cell: the partial counts of a plane added over its workgroups -> int64 [plane][cells + 1]
//   k_hist_row               a thread per cell: the planes of the armed range added -> the ring slot the host names
//   k_range_partials<Q> / k_range_finish   smallest and largest non-NaN value per plane (fmin / fmax drop a NaN; reduce.h's trees)
// Contention.  A nearly uniform field sends all 64 lanes of a wavefront to one LDS address and the atomics serialise.  Before the
// atomic the wavefront therefore compares every lane's cell with its first lane's (one readfirstlane, one ballot): the lanes that
// agree add their number with ONE atomic, the others add 1 each.  A constant field then costs one atomic per wavefront and value,
// a spread field pays one ballot per value.  Measured on 512^3, interior planes (tools/time_hist.py, profiles/hist_cost.json): uz with
// 128 bins 0.258 ms spread / 0.241 ms constant, q 0.418 / 0.419 ms, (q, uz) 64 x 64 0.693 / 0.705 ms - 4.1 to 5.1 TB/s of the bytes read
// beside a copy probe of 6.3 TB/s read + write.  The kernel without the merge was not measured.
// Shape.  chunk = 8192 * ceil((cells + 1) / 2048) nodes per workgroup: the partial counts (4 B per cell, written once and read
// once) stay below an eighth of the bytes the workgroup reads, and 512^2 planes still give 32 workgroups per plane.  The grid is
// free - counts are integers - so this is a choice of traffic, not of result.  The figures above are this rule's (32, 32 and 11
// workgroups per plane); no other chunk was measured.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "reduce.h"
#include "ring.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int HIST_THREADS = 256;
constexpr int HIST_LOADS = 16;           // loads in flight per thread and tile
constexpr long long HIST_CHUNK0 = 8192;  // nodes: HIST_THREADS * HIST_LOADS * 2 (a 16 B tile of one array)
constexpr int NVALUES = EKPNP_NFIELDS + 1;

static const char* const kValueNames[NVALUES] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T", "q"};

// THE definition (include/ekpnp.h): -1 NaN, 0 underflow, n + 1 overflow, else 1 + min((int)((v - lo) * scale), n - 1)
__host__ __device__ __forceinline__ int hist_index(double lo, double hi, double scale, int n, double v) {
  if (v != v) return -1;
  if (v < lo) return 0;
  if (v >= hi) return n + 1;
  const double d = v - lo;
  const double s = d * scale;
  int k = (int)s;
  if (k > n - 1) k = n - 1;
  return 1 + k;
}

struct HistAxisDev {
  double lo, hi, scale;
  int n;
};
struct HistArgs {
  const double* a0;  // plane 0 of the launch: the field of axis a, or c when it is q ...
  const double* a1;  // ... and cn
  const double* b0;
  const double* b1;
  HistAxisDev A, B;
  long long plane, chunk;
  int cells;  // the counter behind the cells, index `cells`, is nonfinite
  int nb2;    // b.n + 2 (1 for a 1-D spec)
};

// one value's cell: the lanes that agree with the wavefront's first lane add their number at once (cell < 0: nothing to add)
__device__ __forceinline__ void hist_add(unsigned* cnt, int cell) {
  const int lead = __builtin_amdgcn_readfirstlane(cell);
  const bool same = cell == lead;
  const unsigned long long m = __ballot(same);
  if (same) {
    if (lead >= 0 && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&cnt[lead], (unsigned)__popcll(m));
  } else if (cell >= 0) {
    atomicAdd(&cnt[cell], 1u);
  }
}

template <bool TWO_D, bool QA, bool QB, int VEC>
__device__ __forceinline__ void hist_chunk(const HistArgs& a, const double* __restrict__ a0, const double* __restrict__ a1, const double* __restrict__ b0,
                                           const double* __restrict__ b1, long long begin, long long end, unsigned* cnt) {
  constexpr int NARR = (QA ? 2 : 1) + (TWO_D ? (QB ? 2 : 1) : 0);
  constexpr int L = NARR == 1 ? HIST_LOADS : NARR == 2 ? HIST_LOADS / 2 : HIST_LOADS / 4;
  constexpr int N = L * VEC;
  constexpr long long TILE = (long long)HIST_THREADS * N;
  for (long long t0 = begin; t0 < end; t0 += TILE) {
    double xa[N], ya[QA ? N : 1], xb[TWO_D ? N : 1], yb[TWO_D && QB ? N : 1];
#pragma unroll
    for (int k = 0; k < L; ++k) {
      const long long i = t0 + ((long long)k * HIST_THREADS + threadIdx.x) * VEC;
      if constexpr (VEC == 2) {  // (begin and TILE are even: i is, and a0 + i is 16-byte aligned)
        const bool two = i + 1 < end, one = i < end;
        double2 v = two ? *(const double2*)(a0 + i) : double2{one ? a0[i] : 0.0, 0.0};
        xa[2 * k] = v.x; xa[2 * k + 1] = v.y;
        if constexpr (QA) { v = two ? *(const double2*)(a1 + i) : double2{one ? a1[i] : 0.0, 0.0}; ya[2 * k] = v.x; ya[2 * k + 1] = v.y; }
        if constexpr (TWO_D) { v = two ? *(const double2*)(b0 + i) : double2{one ? b0[i] : 0.0, 0.0}; xb[2 * k] = v.x; xb[2 * k + 1] = v.y; }
        if constexpr (TWO_D && QB) { v = two ? *(const double2*)(b1 + i) : double2{one ? b1[i] : 0.0, 0.0}; yb[2 * k] = v.x; yb[2 * k + 1] = v.y; }
      } else {
        const bool one = i < end;
        xa[k] = one ? a0[i] : 0.0;
        if constexpr (QA) ya[k] = one ? a1[i] : 0.0;
        if constexpr (TWO_D) xb[k] = one ? b0[i] : 0.0;
        if constexpr (TWO_D && QB) yb[k] = one ? b1[i] : 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < L; ++k) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int j = k * VEC + e;
        const long long i = t0 + ((long long)k * HIST_THREADS + threadIdx.x) * VEC + e;
        double va = xa[j];
        if constexpr (QA) va = va - ya[j];
        const int ia = hist_index(a.A.lo, a.A.hi, a.A.scale, a.A.n, va);
        int cell;
        if constexpr (TWO_D) {
          double vb = xb[j];
          if constexpr (QB) vb = vb - yb[j];
          const int ib = hist_index(a.B.lo, a.B.hi, a.B.scale, a.B.n, vb);
          cell = (ia < 0 || ib < 0) ? a.cells : ia * a.nb2 + ib;
        } else {
          cell = ia < 0 ? a.cells : ia;
        }
        hist_add(cnt, i < end ? cell : -1);
      }
    }
  }
}

// partial[(z * gridDim.x + b) * (cells + 1) + cell]
template <bool TWO_D, bool QA, bool QB>
__global__ void __launch_bounds__(HIST_THREADS) k_hist_partials(HistArgs a, unsigned* __restrict__ partial) {
  extern __shared__ unsigned hist_cnt[];
  const int stride = a.cells + 1;
  for (int i = threadIdx.x; i < stride; i += HIST_THREADS) hist_cnt[i] = 0u;
  __syncthreads();
  const long long zoff = (long long)blockIdx.y * a.plane;
  const double* a0 = a.a0 + zoff;
  const double* a1 = QA ? a.a1 + zoff : a0;
  const double* b0 = TWO_D ? a.b0 + zoff : a0;
  const double* b1 = TWO_D && QB ? a.b1 + zoff : a0;
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.plane ? begin + a.chunk : a.plane;
  const bool aligned = (((uintptr_t)a0 | (uintptr_t)a1 | (uintptr_t)b0 | (uintptr_t)b1) & 15) == 0;
  if (aligned) hist_chunk<TWO_D, QA, QB, 2>(a, a0, a1, b0, b1, begin, end, hist_cnt);
  else hist_chunk<TWO_D, QA, QB, 1>(a, a0, a1, b0, b1, begin, end, hist_cnt);
  __syncthreads();
  unsigned* out = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * stride;
  for (int i = threadIdx.x; i < stride; i += HIST_THREADS) out[i] = hist_cnt[i];
}

// planes[z * stride + cell] = the plane's partial counts added over its workgroups (eight loads in flight)
__global__ void __launch_bounds__(HIST_THREADS) k_hist_finish(const unsigned* __restrict__ partial, int nwg, int stride, long long* __restrict__ planes) {
  const int cell = blockIdx.x * HIST_THREADS + threadIdx.x, z = blockIdx.y;
  if (cell >= stride) return;
  const unsigned* p = partial + (long long)z * nwg * stride + cell;
  long long r = 0;
  for (int b0 = 0; b0 < nwg; b0 += 8) {
    unsigned v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = b0 + k < nwg ? p[(long long)(b0 + k) * stride] : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) r += (long long)v[k];
  }
  planes[(long long)z * stride + cell] = r;
}

// row[cell] = planes[0 .. np - 1][cell] added (eight loads in flight)
__global__ void __launch_bounds__(HIST_THREADS) k_hist_row(const long long* __restrict__ planes, int np, int stride, long long* __restrict__ row) {
  const int cell = blockIdx.x * HIST_THREADS + threadIdx.x;
  if (cell >= stride) return;
  const long long* p = planes + cell;
  long long r = 0;
  for (int z0 = 0; z0 < np; z0 += 8) {
    long long v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = z0 + k < np ? p[(long long)(z0 + k) * stride] : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) r += v[k];
  }
  row[cell] = r;
}

__device__ __forceinline__ double wave_min(double v) { return -wave_max(-v); }

// partial[(z * gridDim.x + b) * 2 + {0: min, 1: max}] of the workgroup's 4096 nodes; a NaN is dropped by fmin / fmax
template <bool Q>
__global__ void __launch_bounds__(HIST_THREADS) k_range_partials(const double* __restrict__ f0, const double* __restrict__ f1, long long plane,
                                                                 double* __restrict__ partial) {
  __shared__ double lds[2][HIST_THREADS / 64];
  const long long zoff = (long long)blockIdx.y * plane;
  const long long first = (long long)blockIdx.x * (HIST_THREADS * HIST_LOADS) + threadIdx.x;
  double x[HIST_LOADS], y[Q ? HIST_LOADS : 1];
#pragma unroll
  for (int k = 0; k < HIST_LOADS; ++k) {
    const long long i = first + (long long)k * HIST_THREADS;
    x[k] = i < plane ? f0[zoff + i] : NAN;
    if constexpr (Q) y[k] = i < plane ? f1[zoff + i] : NAN;
  }
  double lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int k = 0; k < HIST_LOADS; ++k) {
    double v = x[k];
    if constexpr (Q) v = v - y[k];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { lds[0][wave] = lo; lds[1][wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < HIST_THREADS / 64; ++w) { lo = fmin(lo, lds[0][w]); hi = fmax(hi, lds[1][w]); }
    double* o = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

// out[z * 2 + {0, 1}]: one wavefront per plane over the plane's workgroups
__global__ void __launch_bounds__(64) k_range_finish(const double* __restrict__ partial, int nwg, double* __restrict__ out) {
  const int z = blockIdx.x;
  const double* p = partial + (long long)z * nwg * 2;
  double lo = INFINITY, hi = -INFINITY;
  for (int b = threadIdx.x; b < nwg; b += 64) { lo = fmin(lo, p[2 * b]); hi = fmax(hi, p[2 * b + 1]); }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (threadIdx.x == 0) { out[2 * z] = lo; out[2 * z + 1] = hi; }
}

// Host side of a context's histograms: made by the first ekpnp_hist_planes / ekpnp_value_range / ekpnp_hist_arm, never by a context that uses none.
struct HistState {
  void* part = nullptr;         // the workgroups' partial counts (or partial ranges); grows to the largest spec seen
  size_t part_bytes = 0;
  long long* planes = nullptr;  // [planes][cells + 1] of the last pass (or [planes][2] doubles of a range)
  size_t planes_bytes = 0;
  Ring ring;                    // rows of [cells + 1] long long
  ekpnp_hist_spec spec{};
  int z_lo = 0, z_hi = 0;
};

static bool axis_ok(const ekpnp_hist_axis& x, const char* which, std::string& err) {
  const std::string w = std::string("hist: axis ") + which + ": ";
  char num[96];
  if (x.value < 0 || x.value >= NVALUES) { err = w + "value = " + std::to_string(x.value) + " outside 0 .. 11"; return false; }
  if (x.n < 1) { err = w + "n = " + std::to_string(x.n) + " (must be >= 1)"; return false; }
  if (!std::isfinite(x.lo)) { std::snprintf(num, sizeof num, "lo = %.17g (must be finite)", x.lo); err = w + num; return false; }
  if (!std::isfinite(x.hi)) { std::snprintf(num, sizeof num, "hi = %.17g (must be finite)", x.hi); err = w + num; return false; }
  if (!(x.hi > x.lo)) { std::snprintf(num, sizeof num, "hi = %.17g is not above lo = %.17g", x.hi, x.lo); err = w + num; return false; }
  const double width = x.hi - x.lo, scale = (double)x.n / width;
  if (!std::isfinite(width) || !std::isfinite(scale)) {
    std::snprintf(num, sizeof num, "n / (hi - lo) = %d / %.17g is not finite", x.n, width);
    err = w + num;
    return false;
  }
  return true;
}

int hist_check_spec(const ekpnp_params& p, const ekpnp_hist_spec* s, std::string& err) {
  if (!s) { err = "hist: NULL spec"; return EKPNP_ERR_INVALID; }
  if (p.nx < 1 || p.ny < 1) { err = "hist: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (!axis_ok(s->a, "a", err)) return EKPNP_ERR_INVALID;
  if (s->b.n != 0 && !axis_ok(s->b, "b", err)) return EKPNP_ERR_INVALID;
  const long long bins = (long long)s->a.n * (s->b.n ? s->b.n : 1);
  if (bins > EKPNP_HIST_MAX_BINS) {
    err = "hist: a.n * max(b.n, 1) = " + std::to_string(s->a.n) + " * " + std::to_string(s->b.n ? s->b.n : 1) + " = " + std::to_string(bins) + " above " +
          std::to_string(EKPNP_HIST_MAX_BINS);
    return EKPNP_ERR_INVALID;
  }
  return EKPNP_OK;
}

int hist_check_range(const ekpnp_params& p, int z_lo, int z_hi, int capacity, std::string& err) {
  if (z_lo < 0) { err = "hist: z_lo = " + std::to_string(z_lo) + " (must be >= 0)"; return EKPNP_ERR_INVALID; }
  if (z_lo > z_hi) { err = "hist: z_lo = " + std::to_string(z_lo) + " above z_hi = " + std::to_string(z_hi); return EKPNP_ERR_INVALID; }
  if (z_hi >= p.nz) { err = "hist: z_hi = " + std::to_string(z_hi) + " outside 0 .. " + std::to_string(p.nz - 1); return EKPNP_ERR_INVALID; }
  if (capacity < 1) { err = "hist: capacity = " + std::to_string(capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

int hist_cells(const ekpnp_hist_spec& s) { return (s.a.n + 2) * (s.b.n ? s.b.n + 2 : 1); }

const ekpnp_hist_spec* hist_armed_spec(const Ctx& c, int* z_lo, int* z_hi) {
  if (!c.hist || !c.hist->ring.ever_armed) return nullptr;
  if (z_lo) *z_lo = c.hist->z_lo;
  if (z_hi) *z_hi = c.hist->z_hi;
  return &c.hist->spec;
}

bool hist_armed(const Ctx& c) { return c.hist && c.hist->ring.armed; }

void hist_release(Ctx& c) {
  if (!c.hist) return;
  if (c.hist->part) (void)hipFree(c.hist->part);
  if (c.hist->planes) (void)hipFree(c.hist->planes);
  ring_release(c.hist->ring);
  delete c.hist;
  c.hist = nullptr;
}

int hist_write_file(const char* path, const ekpnp_params& p, const ekpnp_hist_spec& spec, int z_lo, int z_hi, int64_t recorded, int64_t dropped, int n,
                    const int64_t* steps, const double* times, const int64_t* counts, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open hist file"; return EKPNP_ERR_INVALID; }
  std::fprintf(f, "# ekpnp hist nx %d ny %d nz %d a %s %d %.17g %.17g", p.nx, p.ny, p.nz, kValueNames[spec.a.value], spec.a.n, spec.a.lo, spec.a.hi);
  if (spec.b.n) std::fprintf(f, " b %s %d %.17g %.17g", kValueNames[spec.b.value], spec.b.n, spec.b.lo, spec.b.hi);
  std::fprintf(f, " z_lo %d z_hi %d recorded %lld dropped %lld\n", z_lo, z_hi, (long long)recorded, (long long)dropped);
  const size_t cells = (size_t)hist_cells(spec);
  for (int r = 0; r < n; ++r) {
    const int64_t* row = counts + (size_t)r * (cells + 1);
    std::fprintf(f, "%lld %.17g %lld", (long long)steps[r], times[r], (long long)row[cells]);
    for (size_t k = 0; k < cells; ++k) std::fprintf(f, " %lld", (long long)row[k]);
    std::fprintf(f, "\n");
  }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on hist file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

}  // namespace ekpnp

static inline long long hist_chunk_nodes(int stride) { return HIST_CHUNK0 * (((long long)stride + 2047) / 2048); }
static inline int hist_workgroups(const Ctx& c, long long chunk) { return (int)(((long long)c.plane + chunk - 1) / chunk); }
static inline int range_workgroups(const Ctx& c) { return (int)(((long long)c.plane + HIST_THREADS * HIST_LOADS - 1) / (HIST_THREADS * HIST_LOADS)); }

static int need_hist(Ctx& c) {
  if (c.hist) return EKPNP_OK;
  if (c.nzl > 65535) return fail(c, "hist: more than 65535 planes in one context");
  c.hist = new (std::nothrow) HistState();
  if (!c.hist) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  return EKPNP_OK;
}

// the two scratch buffers at least this large; growing waits for the stream first (a pass of an earlier call may still read them)
static int hist_scratch(Ctx& c, size_t part_bytes, size_t planes_bytes) {
  HistState& h = *c.hist;
  if (part_bytes <= h.part_bytes && planes_bytes <= h.planes_bytes) return EKPNP_OK;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  if (part_bytes > h.part_bytes) {
    if (h.part) { (void)hipFree(h.part); c.bytes -= h.part_bytes; h.part = nullptr; h.part_bytes = 0; }
    HIPCHK(c, hipMalloc(&h.part, part_bytes));
    h.part_bytes = part_bytes;
    c.bytes += part_bytes;
  }
  if (planes_bytes > h.planes_bytes) {
    if (h.planes) { (void)hipFree(h.planes); c.bytes -= h.planes_bytes; h.planes = nullptr; h.planes_bytes = 0; }
    HIPCHK(c, hipMalloc((void**)&h.planes, planes_bytes));
    h.planes_bytes = planes_bytes;
    c.bytes += planes_bytes;
  }
  return EKPNP_OK;
}

static size_t hist_part_bytes(const Ctx& c, const ekpnp_hist_spec& s, int np) {
  const int stride = hist_cells(s) + 1;
  return (size_t)np * (size_t)hist_workgroups(c, hist_chunk_nodes(stride)) * (size_t)stride * sizeof(unsigned);
}

static bool value_needs_efield(int v) { return v == EKPNP_PHI || v == EKPNP_EX || v == EKPNP_EY || v == EKPNP_EZ; }

// enqueue the counts of the local planes zl0 .. zl0 + np - 1 into HistState::planes ([np][cells + 1]); the scratch is large enough
static int hist_enqueue(Ctx& c, const ekpnp_hist_spec& s, int zl0, int np) {
  HistState& h = *c.hist;
  const bool two = s.b.n != 0;
  if (value_needs_efield(s.a.value) || (two && value_needs_efield(s.b.value))) {
    if (int rc = ensure_efield(c)) return rc;  // the arrays as ekpnp_get_field would return them
  }
  const bool qa = s.a.value == EKPNP_HIST_Q, qb = two && s.b.value == EKPNP_HIST_Q;
  const size_t off = (size_t)zl0 * c.plane;
  const int cells = hist_cells(s), stride = cells + 1;
  HistArgs a{};
  a.a0 = (qa ? c.fld[EKPNP_C] : c.fld[s.a.value]) + off;
  a.a1 = qa ? c.fld[EKPNP_CN] + off : a.a0;
  a.b0 = two ? (qb ? c.fld[EKPNP_C] : c.fld[s.b.value]) + off : a.a0;
  a.b1 = qb ? c.fld[EKPNP_CN] + off : a.a0;
  a.A = HistAxisDev{s.a.lo, s.a.hi, (double)s.a.n / (s.a.hi - s.a.lo), s.a.n};
  a.B = two ? HistAxisDev{s.b.lo, s.b.hi, (double)s.b.n / (s.b.hi - s.b.lo), s.b.n} : a.A;
  a.plane = (long long)c.plane;
  a.chunk = hist_chunk_nodes(stride);
  a.cells = cells;
  a.nb2 = two ? s.b.n + 2 : 1;
  const int nwg = hist_workgroups(c, a.chunk);
  const dim3 grid(nwg, np), block(HIST_THREADS);
  const size_t lds = (size_t)stride * sizeof(unsigned);
  unsigned* part = (unsigned*)h.part;
#define HIST_LAUNCH(T, A, B) hipLaunchKernelGGL((k_hist_partials<T, A, B>), grid, block, lds, c.stream, a, part)
  if (!two) {
    if (qa) HIST_LAUNCH(false, true, false);
    else HIST_LAUNCH(false, false, false);
  } else if (qa) {
    if (qb) HIST_LAUNCH(true, true, true);
    else HIST_LAUNCH(true, true, false);
  } else {
    if (qb) HIST_LAUNCH(true, false, true);
    else HIST_LAUNCH(true, false, false);
  }
#undef HIST_LAUNCH
  note_launch(c, "k_hist_partials");
  hipLaunchKernelGGL(k_hist_finish, dim3((stride + HIST_THREADS - 1) / HIST_THREADS, np), dim3(HIST_THREADS), 0, c.stream, part, nwg, stride, h.planes);
  note_launch(c, "k_hist_finish");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_hist_bin(double lo, double hi, int n, double v) {
  if (n < 1 || !std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return -2;
  const double width = hi - lo, scale = (double)n / width;
  if (!std::isfinite(width) || !std::isfinite(scale)) return -2;
  return hist_index(lo, hi, scale, n, v);
}

extern "C" int ekpnp_hist_spec_check(const ekpnp_params* p, const ekpnp_hist_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "hist: NULL parameters";
  else rc = hist_check_spec(*p, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_hist_range_check(const ekpnp_params* p, int z_lo, int z_hi, int capacity) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "hist: NULL parameters";
  else rc = hist_check_range(*p, z_lo, z_hi, capacity, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_hist_planes(ekpnp_ctx* ctx, const ekpnp_hist_spec* spec, int64_t* counts, int64_t* nonfinite) {
  NEEDCTX(ctx);
  if (!counts || !nonfinite) return fail(c, "NULL pointer");
  if (int rc = hist_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = need_hist(c)) return rc;
  const size_t cells = (size_t)hist_cells(*spec), stride = cells + 1;
  if (int rc = hist_scratch(c, hist_part_bytes(c, *spec, c.nzl), (size_t)c.nzl * stride * sizeof(long long))) return rc;
  if (int rc = hist_enqueue(c, *spec, 0, c.nzl)) return rc;
  std::vector<int64_t> rows((size_t)c.nzl * stride);
  HIPCHK(c, hipMemcpyAsync(rows.data(), c.hist->planes, rows.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  for (int z = 0; z < c.nzl; ++z) {
    const int64_t* r = rows.data() + (size_t)z * stride;
    for (size_t k = 0; k < cells; ++k) counts[(size_t)z * cells + k] = r[k];
    nonfinite[z] = r[cells];
  }
  return EKPNP_OK;
}

extern "C" int ekpnp_value_range(ekpnp_ctx* ctx, int value, double* vmin, double* vmax) {
  NEEDCTX(ctx);
  if (!vmin || !vmax) return fail(c, "NULL pointer");
  if (value < 0 || value >= NVALUES) { c.err = "hist: value = " + std::to_string(value) + " outside 0 .. 11"; return EKPNP_ERR_INVALID; }
  if (int rc = need_hist(c)) return rc;
  const int nwg = range_workgroups(c);
  if (int rc = hist_scratch(c, (size_t)c.nzl * nwg * 2 * sizeof(double), (size_t)c.nzl * 2 * sizeof(double))) return rc;
  if (value_needs_efield(value))
    if (int rc = ensure_efield(c)) return rc;
  const dim3 grid(nwg, c.nzl), block(HIST_THREADS);
  double* part = (double*)c.hist->part;
  double* out = (double*)c.hist->planes;
  if (value == EKPNP_HIST_Q) hipLaunchKernelGGL((k_range_partials<true>), grid, block, 0, c.stream, c.fld[EKPNP_C], c.fld[EKPNP_CN], (long long)c.plane, part);
  else hipLaunchKernelGGL((k_range_partials<false>), grid, block, 0, c.stream, c.fld[value], c.fld[value], (long long)c.plane, part);
  note_launch(c, "k_range_partials");
  hipLaunchKernelGGL(k_range_finish, dim3(c.nzl), dim3(64), 0, c.stream, part, nwg, out);
  note_launch(c, "k_range_finish");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  std::vector<double> mm((size_t)c.nzl * 2);
  HIPCHK(c, hipMemcpyAsync(mm.data(), out, mm.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  for (int z = 0; z < c.nzl; ++z) { vmin[z] = mm[2 * (size_t)z]; vmax[z] = mm[2 * (size_t)z + 1]; }
  return EKPNP_OK;
}

extern "C" int ekpnp_hist_arm(ekpnp_ctx* ctx, const ekpnp_hist_spec* spec, int z_lo, int z_hi, int capacity) {
  NEEDCTX(ctx);
  if (int rc = hist_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = hist_check_range(c.p, z_lo, z_hi, capacity, c.err)) return rc;
  if (int rc = need_hist(c)) return rc;
  HistState& h = *c.hist;
  h.ring.armed = false;
  const size_t stride = (size_t)hist_cells(*spec) + 1;
  const int lo = z_lo > c.z0 ? z_lo : c.z0, hi = z_hi < c.z0 + c.nzl - 1 ? z_hi : c.z0 + c.nzl - 1;
  const int np = hi >= lo ? hi - lo + 1 : 0;  // this context's part of the range; 0: its rows are zeros
  if (np > 0)
    if (int rc = hist_scratch(c, hist_part_bytes(c, *spec, np), (size_t)np * stride * sizeof(long long))) return rc;
  h.spec = *spec;
  h.z_lo = z_lo;
  h.z_hi = z_hi;
  return ring_arm(c, h.ring, capacity, stride * sizeof(long long));
}

extern "C" int ekpnp_hist_disarm(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (c.hist) c.hist->ring.armed = false;  // the ring and its rows stay readable until the next arm
  return EKPNP_OK;
}

extern "C" int ekpnp_hist_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDCTX(ctx);
  if (!c.hist || !c.hist->ring.armed) return fail(c, "ekpnp_hist_record: no histogram armed");
  HistState& h = *c.hist;
  const size_t stride = (size_t)hist_cells(h.spec) + 1;
  long long* row = (long long*)ring_next_row(h.ring);
  const int lo = h.z_lo > c.z0 ? h.z_lo : c.z0, hi = h.z_hi < c.z0 + c.nzl - 1 ? h.z_hi : c.z0 + c.nzl - 1;
  if (hi < lo) {  // no plane of the range here: a row of zeros, no kernel reads a field
    HIPCHK(c, hipMemsetAsync(row, 0, stride * sizeof(long long), c.stream));
  } else {
    const int np = hi - lo + 1;
    if (int rc = hist_scratch(c, hist_part_bytes(c, h.spec, np), (size_t)np * stride * sizeof(long long))) return rc;  // (a synchronous call never shrinks them: no wait)
    if (int rc = hist_enqueue(c, h.spec, lo - c.z0, np)) return rc;
    hipLaunchKernelGGL(k_hist_row, dim3(((int)stride + HIST_THREADS - 1) / HIST_THREADS), dim3(HIST_THREADS), 0, c.stream, h.planes, np, (int)stride, row);
    note_launch(c, "k_hist_row");
    if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  }
  ring_note_row(h.ring, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_hist_count(const ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  if (!ctx) return EKPNP_ERR_INVALID;
  ring_count(ctx->c.hist ? &ctx->c.hist->ring : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_hist_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, int64_t* counts) {
  NEEDCTX(ctx);
  return ring_read(c, c.hist ? &c.hist->ring : nullptr, "ekpnp_hist_read", first, count, steps, times, counts);
}

extern "C" int ekpnp_hist_save(ekpnp_ctx* ctx, const char* path) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  int z_lo = 0, z_hi = 0;
  const ekpnp_hist_spec* spec = hist_armed_spec(c, &z_lo, &z_hi);
  if (!spec) return fail(c, "ekpnp_hist_save: no histogram was armed");
  int64_t rec = 0, dropped = 0;
  (void)ekpnp_hist_count(ctx, &rec, &dropped);
  const int n = (int)(rec - dropped);
  std::vector<int64_t> steps((size_t)n), counts((size_t)n * ((size_t)hist_cells(*spec) + 1));
  std::vector<double> times((size_t)n);
  if (int rc = ekpnp_hist_read(ctx, 0, n, steps.data(), times.data(), counts.data())) return rc;
  return hist_write_file(path, c.p, *spec, z_lo, z_hi, rec, dropped, n, steps.data(), times.data(), counts.data(), c.err);
}
