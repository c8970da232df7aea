// stats.hip — on-device plane profiles and running statistics (include/ekpnp.h: ekpnp_plane_sums, ekpnp_stats_*,
// ekpnp_save_profiles; no reference counterpart).
//
// What a channel-flow run is plotted by - plane sums of the eleven fields, of their squares and of the flux / body-force
// products, EKPNP_NPROFILES = 24 per plane - used to cost eleven ekpnp_get_field copies and a host loop, the pattern diag.hip
// removed for current() and record_umax (main.cu:211-222).  Here:
//   k_plane_partials   grid (ceil(nx*ny / STATS_CHUNK), nzl): a workgroup reads STATS_CHUNK consecutive nodes of ONE plane from
//                      each of the eleven arrays once (88 B per node) and stores its 24 partial sums
//   k_plane_finish     one workgroup per plane: adds the partial sums of the plane in ascending workgroup order into
//                      [EKPNP_NPROFILES][nzl], and on request adds that to the running sums (ekpnp_stats_accumulate)
// As in diag.hip: wave64 shuffle trees, one LDS slot per wave, no atomics.  The order in which the terms of a plane are added
// depends on nx*ny alone - thread t of workgroup b takes nodes b*STATS_CHUNK + k*256 + t, k ascending; fixed trees over lanes
// and waves; partial sums in ascending b - not on z0, nzl, the device or the buffer mode: a plane's sums are the same bits in a
// single, an in-place and a slab context.
#include <cstdio>
#include <vector>

#include "ekpnp_internal.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int STATS_THREADS = 256;
constexpr int STATS_PER_THREAD = 16;
constexpr int STATS_CHUNK = STATS_THREADS * STATS_PER_THREAD;  // nodes of a plane per workgroup
constexpr int NP = EKPNP_NPROFILES;

struct StatsFields {
  const double* f[EKPNP_NFIELDS];
};

__device__ __forceinline__ double stats_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(STATS_THREADS) k_plane_partials(StatsFields a, long long plane, double* __restrict__ partial) {
  __shared__ double lds[NP][STATS_THREADS / 64];
  const long long first = (long long)blockIdx.x * STATS_CHUNK + threadIdx.x;
  const long long zoff = (long long)blockIdx.y * plane;
  double s[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) s[q] = 0.0;
#pragma unroll 4
  for (int k = 0; k < STATS_PER_THREAD; ++k) {
    const long long i = first + (long long)k * STATS_THREADS;
    if (i < plane) {
      const long long t = zoff + i;
      double v[EKPNP_NFIELDS];
#pragma unroll
      for (int q = 0; q < EKPNP_NFIELDS; ++q) v[q] = a.f[q][t];
#pragma unroll
      for (int q = 0; q < EKPNP_NFIELDS; ++q) s[q] += v[q];
      const double c = v[EKPNP_C], cn = v[EKPNP_CN], T = v[EKPNP_T];
      const double ux = v[EKPNP_UX], uy = v[EKPNP_UY], uz = v[EKPNP_UZ];
      const double qd = c - cn;
      s[EKPNP_PROF_UX_UX] += ux * ux;
      s[EKPNP_PROF_UY_UY] += uy * uy;
      s[EKPNP_PROF_UZ_UZ] += uz * uz;
      s[EKPNP_PROF_C_C] += c * c;
      s[EKPNP_PROF_CN_CN] += cn * cn;
      s[EKPNP_PROF_T_T] += T * T;
      s[EKPNP_PROF_UZ_T] += uz * T;
      s[EKPNP_PROF_UZ_C] += uz * c;
      s[EKPNP_PROF_UZ_CN] += uz * cn;
      s[EKPNP_PROF_Q_EX] += qd * v[EKPNP_EX];
      s[EKPNP_PROF_Q_EZ] += qd * v[EKPNP_EZ];
      s[EKPNP_PROF_UX_UZ] += ux * uz;
      s[EKPNP_PROF_Q_Q] += qd * qd;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const double r = stats_wave_sum(s[q]);
    if (lane == 0) lds[q][wave] = r;
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    double r = lds[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < STATS_THREADS / 64; ++w) r += lds[threadIdx.x][w];
    partial[((long long)blockIdx.y * gridDim.x + blockIdx.x) * NP + threadIdx.x] = r;
  }
}

// out[q][z] = the plane's partial sums in ascending workgroup order; acc[q][z] = acc[q][z] + out[q][z] when asked for
__global__ void __launch_bounds__(64) k_plane_finish(const double* __restrict__ partial, int nwg, int nzl, double* __restrict__ out,
                                                     double* __restrict__ acc) {
  const int z = blockIdx.x, q = threadIdx.x;
  if (q >= NP) return;
  const double* p = partial + (long long)z * nwg * NP + q;
  double r = 0.0;
  for (int b = 0; b < nwg; ++b) r += p[(long long)b * NP];
  const long long o = (long long)q * nzl + z;
  out[o] = r;
  if (acc) acc[o] = acc[o] + r;
}

int stats_workgroups_per_plane(const Ctx& c) { return (int)(((long long)c.plane + STATS_CHUNK - 1) / STATS_CHUNK); }

void launch_plane_sums(Ctx& c, double* acc) {
  const int nwg = stats_workgroups_per_plane(c);
  StatsFields a;
  for (int i = 0; i < EKPNP_NFIELDS; ++i) a.f[i] = c.fld[i];
  hipLaunchKernelGGL(k_plane_partials, dim3(nwg, c.nzl), dim3(STATS_THREADS), 0, c.stream, a, (long long)c.plane, c.stats_part);
  note_launch(c, "k_plane_partials");
  hipLaunchKernelGGL(k_plane_finish, dim3(c.nzl), dim3(64), 0, c.stream, c.stats_part, nwg, c.nzl, c.stats_out, acc);
  note_launch(c, "k_plane_finish");
}

static const char* const kProfileNames[NP] = {"rho",   "c",   "cn",   "phi", "ux",  "uy",   "uz",   "Ex",   "Ey",    "Ez",  "T",   "ux_ux",
                                              "uy_uy", "uz_uz", "c_c", "cn_cn", "T_T", "uz_T", "uz_c", "uz_cn", "q_Ex", "q_Ez", "ux_uz", "q_q"};

int stats_write_file(const char* path, const ekpnp_params& p, int z0, int nzl, int samples, double time, const double* sums, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open profiles file"; return EKPNP_ERR_INVALID; }
  std::fprintf(f, "# ekpnp profiles nx %d ny %d nz %d z0 %d nz_local %d samples %d time %.17g\n", p.nx, p.ny, p.nz, z0, nzl, samples, time);
  std::fprintf(f, "# z zcoord");
  for (int q = 0; q < NP; ++q) std::fprintf(f, " %s", kProfileNames[q]);
  std::fprintf(f, "\n");
  const double nodes = (double)((long long)p.nx * p.ny);
  const double denom = samples > 0 ? (double)samples * nodes : nodes;
  for (int z = 0; z < nzl; ++z) {
    std::fprintf(f, "%d %.17g", z0 + z, (double)(z0 + z) * p.dz);
    for (int q = 0; q < NP; ++q) std::fprintf(f, " %.17g", sums[(size_t)q * nzl + z] / denom);
    std::fprintf(f, "\n");
  }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on profiles file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

}  // namespace ekpnp

static inline size_t stats_entries(const Ctx& c) { return (size_t)NP * (size_t)c.nzl; }

// the three arrays, once: [partials | sums of the last pass | running sums]
static int need_stats(Ctx& c) {
  if (c.stats_part) return EKPNP_OK;
  if (c.nzl > 65535) return fail(c, "plane profiles: more than 65535 planes in one context");
  const size_t npart = (size_t)c.nzl * (size_t)stats_workgroups_per_plane(c) * NP, n = stats_entries(c);
  const size_t bytes = (npart + 2 * n) * sizeof(double);
  double* base = nullptr;
  HIPCHK(c, hipMalloc((void**)&base, bytes));
  hipError_t e = hipMemsetAsync(base + npart, 0, 2 * n * sizeof(double), c.stream);
  if (e != hipSuccess) {
    (void)hipFree(base);
    HIPCHK(c, e);
  }
  c.stats_part = base;
  c.stats_out = base + npart;
  c.stats_acc = base + npart + n;
  c.stats_samples = 0;
  c.bytes += bytes;
  return EKPNP_OK;
}

// enqueue one pass over the current fields (phi and E are read from their arrays: a lazy solve's E first)
static int enqueue_plane_sums(Ctx& c, bool accumulate) {
  int rc = need_stats(c);
  if (rc) return rc;
  if ((rc = ensure_efield(c))) return rc;
  launch_plane_sums(c, accumulate ? c.stats_acc : nullptr);
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_plane_sums(ekpnp_ctx* ctx, double* host_out) {
  NEEDCTX(ctx);
  if (!host_out) return fail(c, "NULL pointer");
  if (int rc = enqueue_plane_sums(c, false)) return rc;
  HIPCHK(c, hipMemcpyAsync(host_out, c.stats_out, stats_entries(c) * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_stats_reset(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (c.stats_acc) HIPCHK(c, hipMemsetAsync(c.stats_acc, 0, stats_entries(c) * sizeof(double), c.stream));
  c.stats_samples = 0;
  return EKPNP_OK;
}

extern "C" int ekpnp_stats_accumulate(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (int rc = enqueue_plane_sums(c, true)) return rc;
  ++c.stats_samples;
  return EKPNP_OK;
}

extern "C" int ekpnp_stats_get(ekpnp_ctx* ctx, double* host_out, int* n_samples) {
  NEEDCTX(ctx);
  if (!host_out || !n_samples) return fail(c, "NULL pointer");
  if (c.stats_acc) {
    HIPCHK(c, hipMemcpyAsync(host_out, c.stats_acc, stats_entries(c) * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(c, hipStreamSynchronize(c.stream));
  } else {
    for (size_t i = 0; i < stats_entries(c); ++i) host_out[i] = 0.0;
  }
  *n_samples = c.stats_samples;
  return EKPNP_OK;
}

extern "C" int ekpnp_save_profiles(ekpnp_ctx* ctx, const char* path, double time) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  std::vector<double> h(stats_entries(c));
  int samples = 0;
  int rc = ekpnp_stats_get(ctx, h.data(), &samples);
  if (rc == EKPNP_OK && samples == 0) rc = ekpnp_plane_sums(ctx, h.data());  // nothing accumulated: the current fields
  if (rc) return rc;
  return stats_write_file(path, c.p, c.z0, c.nzl, samples, time, h.data(), c.err);
}
