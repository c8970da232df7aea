// monitor.hip — per-step scalar time series kept on the device (include/ekpnp.h: ekpnp_monitor_*; no reference counterpart).
//
// The reference takes its time series - the current through the plate, the maximum velocity - every 50 steps because each
// number costs three full-field copies to the host (main.cu:211-222).  diag.hip moved the reductions onto the device, but
// ekpnp_current / ekpnp_umax are complete on return: a stream synchronise, a host round trip and, under lazy E, a pass that
// writes three field arrays.  Here EKPNP_NMONITORS = 11 scalars are reduced after a step and appended to a ring in device
// memory; nothing is waited for, and the ring is read out whenever the host likes.
//   k_monitor_plates   grid (blocks of k_wall_current, 2 plates): the wall current (the terms, the grid-stride loop and the trees
//                      of diag.hip's k_wall_current, so the bits are those of ekpnp_current) and the one-sided wall gradient of
//                      T, of the plates this context holds; reads at most three planes per plate.  Under lazy E the plate's Ez
//                      is formed from phi with the expression of k_phi_efield / the collide's EPHI path (poisson.hip,
//                      lbm_kernels.hip): the E arrays are neither read nor brought up to date.
//   k_monitor_volume   grid (ceil(nx*ny / MON_CHUNK), nzl), the shape of stats.hip's k_plane_partials: a workgroup reads
//                      MON_CHUNK consecutive nodes of ONE plane from the arrays the selected quantities need (at most seven,
//                      56 B per node) and stores its partial sums and maxima
//   k_monitor_planes   one lane per (plane, quantity): the plane's partial results in ascending workgroup order
//   k_monitor_finish   one workgroup: the plates' partial sums as diag.hip's k_final adds them; the plane sums in ascending z;
//                      then the row goes to the ring slot the
//                      DEVICE-side cursor names and the cursor moves on - a replayed hipGraph therefore never reuses a slot.
// No atomics.  The order of the additions depends on nx*ny and on the planes of the context alone, not on the buffer mode, the
// way the step was enqueued (eagerly, graph replay) or "batch_moments".
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "reduce.h"
#include "ring.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int NM = EKPNP_NMONITORS;
constexpr int MON_THREADS = 256;
constexpr int MON_PER_THREAD = 16;
constexpr int MON_CHUNK = MON_THREADS * MON_PER_THREAD;  // nodes of a plane per workgroup (stats.hip's STATS_CHUNK)
constexpr int MON_PLATE_BLOCKS = 1024;                   // diag.hip's DIAG_BLOCKS
constexpr int MON_NV = 7;                                // per-workgroup results of the volume pass: u_u, q, q_q, uz_T, nonfinite | uz_max, rho_dev
constexpr int MON_NVSUM = 5;                             // the first five are sums, the last two maxima
constexpr int MON_LDS_PLANES = 4096;                     // plane results k_monitor_finish keeps in LDS (32 KB: up to 585 planes)
constexpr uint32_t MON_ALL = (1u << NM) - 1u;
constexpr uint32_t MON_PLATES = 0xFu;                    // ids 0..3
constexpr uint32_t MON_VOLUME = MON_ALL & ~MON_PLATES;   // ids 4..10

static const char* const kMonitorNames[NM] = {"current_top", "current_bottom", "dTdz_bottom", "dTdz_top", "uz_max", "u_u",
                                              "q",           "q_q",            "uz_T",        "rho_dev",  "nonfinite"};

struct MonPlateArgs {
  const double* c;
  const double* cn;
  const double* ez;
  const double* phi;
  const double* T;
  long long plane;
  int nzl;
  int has_top, has_bot;
  uint32_t mask;
  double vlo, vhi, dz;
};

// blockIdx.y = 0: the upper plate (planes nzl-1, nzl-2, nzl-3 of a context that holds it), 1: the lower one (planes 0, 1, 2).
// partial[(2 y + 0) * MON_PLATE_BLOCKS + b]: wall current terms (LBM.cu:2689-2690,2704-2706), [(2 y + 1) ...]: the wall gradient of T.
// PHI: Ez of the plate = gpu_bc's copy of the neighbouring interior plane's Ez (poisson.cu:57-69), 0.5*(phi(z-1) - phi(z+1))/dz with
// the plate's phi taken from voltage / voltage2, as k_phi_efield writes it.
template <bool PHI>
__global__ void __launch_bounds__(256) k_monitor_plates(MonPlateArgs a, double* __restrict__ partial) {
  __shared__ double lds[4];
  const bool top = blockIdx.y == 0;
  if (!(top ? a.has_top : a.has_bot)) return;
  const bool want_i = (a.mask & (top ? 1u : 2u)) != 0, want_t = (a.mask & (top ? 8u : 4u)) != 0;
  const long long w = top ? (long long)(a.nzl - 1) * a.plane : 0;
  const long long n1 = top ? (long long)(a.nzl - 2) * a.plane : a.plane;
  const long long n2 = top ? (long long)(a.nzl - 3) * a.plane : 2 * a.plane;
  double acc = 0.0, acct = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.plane; i += (long long)gridDim.x * blockDim.x) {
    if (want_i) {
      const double ce = 2.0 * a.c[n1 + i] - a.c[n2 + i];
      const double cne = 2.0 * a.cn[n1 + i] - a.cn[n2 + i];
      double e;
      if constexpr (PHI) {
        const double pm = top ? a.phi[n2 + i] : a.vlo, pp = top ? a.vhi : a.phi[n2 + i];
        e = 0.5 * (pm - pp) / a.dz;
      } else {
        e = a.ez[w + i];
      }
      acc += (ce - cne) * e;
    }
    if (want_t) {
      const double t0 = a.T[w + i], t1 = a.T[n1 + i], t2 = a.T[n2 + i];
      acct += top ? (3.0 * t0 - 4.0 * t1 + t2) : (4.0 * t1 - 3.0 * t0 - t2);
    }
  }
  const double r = block_reduce<false>(acc, lds);
  if (threadIdx.x == 0) partial[(2 * blockIdx.y + 0) * MON_PLATE_BLOCKS + blockIdx.x] = r;
  __syncthreads();
  const double rt = block_reduce<false>(acct, lds);
  if (threadIdx.x == 0) partial[(2 * blockIdx.y + 1) * MON_PLATE_BLOCKS + blockIdx.x] = rt;
}

struct MonVolArgs {
  const double* rho;
  const double* c;
  const double* cn;
  const double* T;
  const double* ux;
  const double* uy;
  const double* uz;
  long long plane;
  double rho0;
  uint32_t mask;
};

__global__ void __launch_bounds__(MON_THREADS) k_monitor_volume(MonVolArgs a, double* __restrict__ partial) {
  __shared__ double lds[MON_NV][MON_THREADS / 64];
  // the arrays the selected quantities need (uniform over the launch); an array nobody asked for is not read
  const bool r_rho = (a.mask & ((1u << 9) | (1u << 10))) != 0;
  const bool r_q = (a.mask & ((1u << 6) | (1u << 7) | (1u << 10))) != 0;
  const bool r_t = (a.mask & ((1u << 8) | (1u << 10))) != 0;
  const bool r_uxy = (a.mask & (1u << 5)) != 0;
  const bool r_uz = (a.mask & ((1u << 4) | (1u << 5) | (1u << 8))) != 0;
  const long long first = (long long)blockIdx.x * MON_CHUNK + threadIdx.x;
  const long long zoff = (long long)blockIdx.y * a.plane;
  double s[MON_NV];
#pragma unroll
  for (int q = 0; q < MON_NV; ++q) s[q] = 0.0;
#pragma unroll 4
  for (int k = 0; k < MON_PER_THREAD; ++k) {
    const long long i = first + (long long)k * MON_THREADS;
    if (i < a.plane) {
      const long long t = zoff + i;
      const double rho = r_rho ? a.rho[t] : a.rho0;
      const double c = r_q ? a.c[t] : 0.0, cn = r_q ? a.cn[t] : 0.0;
      const double T = r_t ? a.T[t] : 0.0;
      const double ux = r_uxy ? a.ux[t] : 0.0, uy = r_uxy ? a.uy[t] : 0.0;
      const double uz = r_uz ? a.uz[t] : 0.0;
      const double qd = c - cn;
      s[0] += ux * ux + uy * uy + uz * uz;
      s[1] += qd;
      s[2] += qd * qd;
      s[3] += uz * T;
      const bool fin = isfinite(rho) && isfinite(c) && isfinite(cn) && isfinite(T);
      s[4] += fin ? 0.0 : 1.0;
      s[5] = fmax(s[5], uz);                  // umax starts at 0 (LBM.cu:2718)
      s[6] = fmax(s[6], fabs(rho - a.rho0));  // fmax drops a NaN: it is counted by "nonfinite" instead
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < MON_NV; ++q) {
    const double r = q < MON_NVSUM ? wave_sum(s[q]) : wave_max(s[q]);
    if (lane == 0) lds[q][wave] = r;
  }
  __syncthreads();
  if (threadIdx.x < MON_NV) {
    const int q = threadIdx.x;
    double r = lds[q][0];
#pragma unroll
    for (int w = 1; w < MON_THREADS / 64; ++w) r = q < MON_NVSUM ? r + lds[q][w] : fmax(r, lds[q][w]);
    partial[((long long)blockIdx.x * gridDim.y + blockIdx.y) * MON_NV + q] = r;  // [workgroup][z][q]: k_monitor_finish's lanes, one (z, q) each, read side by side
  }
}

// vplane[z][q] = the partial results of plane z in ascending workgroup order; one (z, q) per lane, which reads side by side with
// its neighbours (partial is [workgroup][z][q]), sixteen loads in flight: the chain of additions is short, the latency is not
__global__ void __launch_bounds__(64) k_monitor_planes(const double* __restrict__ partial, int nwg, int nitems, double* __restrict__ vplane) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= nitems) return;
  const bool is_sum = idx % MON_NV < MON_NVSUM;
  const double* p = partial + idx;
  double r = 0.0;  // (the maxima are of non-negative numbers)
  for (int b0 = 0; b0 < nwg; b0 += 16) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = b0 + k < nwg ? p[(long long)(b0 + k) * nitems] : 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (b0 + k < nwg) r = is_sum ? r + v[k] : fmax(r, v[k]);
  }
  vplane[idx] = r;
}

struct MonFinishArgs {
  const double* ppart;  // [4][MON_PLATE_BLOCKS]
  const double* vpart;  // [nwg][nzl][MON_NV]
  const double* vplane;  // [nzl][MON_NV]
  int nb, nwg, nzl;
  int has_top, has_bot;
  uint32_t mask;
  double K, dz;
  double* ring;                  // [capacity][NM], or null: the row goes to `out`
  unsigned long long* cursor;    // rows appended so far (device side)
  int capacity;
  double* out;
};

__global__ void __launch_bounds__(256) k_monitor_finish(MonFinishArgs a) {
  __shared__ double lds[4];
  __shared__ double row[NM];
  __shared__ double splane[MON_LDS_PLANES];
  if (threadIdx.x < NM) row[threadIdx.x] = 0.0;
  __syncthreads();
  if (a.mask & MON_PLATES) {
    // the four plate sums the way diag.hip's k_final<false> adds the partial sums of k_wall_current
    for (int p = 0; p < 4; ++p) {
      if (!(p < 2 ? a.has_top : a.has_bot)) continue;
      const double* part = a.ppart + p * MON_PLATE_BLOCKS;
      double s = 0.0;
      for (int i = threadIdx.x; i < a.nb; i += blockDim.x) s = s + part[i];
      const double r = block_reduce<false>(s, lds);
      if (threadIdx.x == 0) {
        if (p == 0) row[0] = r * a.K * a.dz * a.dz;  // LBM.cu:2708
        if (p == 1) row[3] = r;
        if (p == 2) row[1] = r * a.K * a.dz * a.dz;
        if (p == 3) row[2] = r;
      }
      __syncthreads();
    }
  }
  if (a.mask & MON_VOLUME) {
    // the plane results of k_monitor_planes, into LDS while they fit (one coalesced round of loads instead of a chain of them) ...
    const int nitems = a.nzl * MON_NV;
    const bool in_lds = nitems <= MON_LDS_PLANES;
    const double* planes = a.vplane;
    if (in_lds) {
      for (int idx = threadIdx.x; idx < nitems; idx += blockDim.x) splane[idx] = a.vplane[idx];
      planes = splane;
    }
    __syncthreads();
    // ... added in ascending z
    if (threadIdx.x < MON_NV) {
      const int q = threadIdx.x;
      double r = planes[q];
#pragma unroll 16
      for (int z = 1; z < a.nzl; ++z) r = q < MON_NVSUM ? r + planes[z * MON_NV + q] : fmax(r, planes[z * MON_NV + q]);
      constexpr int col[MON_NV] = {5, 6, 7, 8, 10, 4, 9};
      row[col[q]] = r;
    }
    __syncthreads();
  }
  unsigned long long cur = 0;
  double* dst = a.out;
  if (a.ring) {
    cur = *a.cursor;
    dst = a.ring + (cur % (unsigned long long)a.capacity) * NM;
  }
  __syncthreads();
  if (threadIdx.x < NM) dst[threadIdx.x] = ((a.mask >> threadIdx.x) & 1u) ? row[threadIdx.x] : 0.0;
  if (a.ring && threadIdx.x == 0) *a.cursor = cur + 1;
}

// Host side of a context's monitor: made by the first ekpnp_monitor_sample / ekpnp_monitor_arm, never by a context that uses neither.
struct MonState {
  double* scratch = nullptr;  // one allocation: [plate partials | volume partials | plane results | one row]
  size_t scratch_bytes = 0;
  double* ppart = nullptr;
  double* vpart = nullptr;
  double* vplane = nullptr;
  double* row = nullptr;
  Ring ring;  // [cursor (16 B header) | rows of [NM] doubles]; Ring::recorded is the device cursor once the stream has drained
  uint32_t mask = MON_ALL;
  int every = 1;
  int64_t steps = 0;  // steps completed through ekpnp_step / ekpnp_group_step since arming
};

static inline int mon_workgroups(const Ctx& c) { return (int)(((long long)c.plane + MON_CHUNK - 1) / MON_CHUNK); }
static inline int mon_plate_blocks(const Ctx& c) {
  return (int)((c.plane + 255) / 256 < (size_t)MON_PLATE_BLOCKS ? (c.plane + 255) / 256 : (size_t)MON_PLATE_BLOCKS);
}

int monitor_check_spec(const ekpnp_monitor_spec* s, std::string& err) {
  if (!s) { err = "monitor: NULL spec"; return EKPNP_ERR_INVALID; }
  if (s->quantities & ~MON_ALL) {
    err = "monitor: quantities = " + std::to_string(s->quantities) + " selects an id above " + std::to_string(NM - 1);
    return EKPNP_ERR_INVALID;
  }
  if (s->every < 1) { err = "monitor: every = " + std::to_string(s->every) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (s->capacity < 1) { err = "monitor: capacity = " + std::to_string(s->capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

int monitor_last_every(const Ctx& c) { return c.mon && c.mon->ring.alloc ? c.mon->every : 0; }
int monitor_every(const Ctx& c) { return c.mon && c.mon->ring.armed ? c.mon->every : 0; }
int monitor_steps_to_sample(const Ctx& c) {
  if (!c.mon || !c.mon->ring.armed) return 0x7fffffff;
  return c.mon->every - (int)(c.mon->steps % c.mon->every);
}

void monitor_release(Ctx& c) {
  if (!c.mon) return;
  if (c.mon->scratch) (void)hipFree(c.mon->scratch);
  ring_release(c.mon->ring);
  delete c.mon;
  c.mon = nullptr;
}

int monitor_write_file(const char* path, const ekpnp_params& p, int every, int64_t recorded, int64_t dropped, int n, const int64_t* steps,
                       const double* times, const double* values, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open monitor file"; return EKPNP_ERR_INVALID; }
  std::fprintf(f, "# ekpnp monitor nx %d ny %d nz %d every %d recorded %lld dropped %lld\n", p.nx, p.ny, p.nz, every, (long long)recorded,
               (long long)dropped);
  std::fprintf(f, "# step time");
  for (int q = 0; q < NM; ++q) std::fprintf(f, " %s", kMonitorNames[q]);
  std::fprintf(f, "\n");
  for (int r = 0; r < n; ++r) {
    std::fprintf(f, "%lld %.17g", (long long)steps[r], times[r]);
    for (int q = 0; q < NM; ++q) std::fprintf(f, " %.17g", values[(size_t)r * NM + q]);
    std::fprintf(f, "\n");
  }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on monitor file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

}  // namespace ekpnp

// the host state and the reduction scratch, once
static int need_monitor(Ctx& c) {
  if (c.mon) return EKPNP_OK;
  if (c.nzl > 65535) return fail(c, "monitor: more than 65535 planes in one context");
  if ((c.z0 == 0 || c.z0 + c.nzl == c.p.nz) && c.nzl < 3) return fail(c, "monitor: a context holding a plate needs 3 planes");
  MonState* m = new (std::nothrow) MonState();
  if (!m) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  const size_t np = (size_t)4 * MON_PLATE_BLOCKS, nv = (size_t)c.nzl * (size_t)mon_workgroups(c) * MON_NV, npl = (size_t)c.nzl * MON_NV;
  m->scratch_bytes = (np + nv + npl + 16) * sizeof(double);
  hipError_t e = hipMalloc((void**)&m->scratch, m->scratch_bytes);
  if (e != hipSuccess) {
    delete m;
    HIPCHK(c, e);
  }
  m->ppart = m->scratch;
  m->vpart = m->ppart + np;
  m->vplane = m->vpart + nv;
  m->row = m->vplane + npl;
  c.bytes += m->scratch_bytes;
  c.mon = m;
  return EKPNP_OK;
}

// Enqueue the reduction of the current fields on the context's stream: into the next ring slot (to_ring) or into MonState::row.
// Nothing is waited for; the E arrays are left as they are (a lazy solve's Ez of the plates comes out of phi).
static int monitor_enqueue(Ctx& c, uint32_t mask, bool to_ring) {
  MonState& m = *c.mon;
  const bool has_top = c.z0 + c.nzl == c.p.nz, has_bot = c.z0 == 0;
  const int nb = mon_plate_blocks(c), nwg = mon_workgroups(c);
  if ((mask & MON_PLATES) && (has_top || has_bot)) {
    const MonPlateArgs a{c.fld[EKPNP_C], c.fld[EKPNP_CN], c.fld[EKPNP_EZ], c.fld[EKPNP_PHI], c.fld[EKPNP_T], (long long)c.plane, c.nzl,
                         has_top ? 1 : 0, has_bot ? 1 : 0, mask, c.p.voltage, c.p.voltage2, c.p.dz};
    if (c.e_stale) hipLaunchKernelGGL((k_monitor_plates<true>), dim3(nb, 2), dim3(256), 0, c.stream, a, m.ppart);
    else hipLaunchKernelGGL((k_monitor_plates<false>), dim3(nb, 2), dim3(256), 0, c.stream, a, m.ppart);
    note_launch(c, "k_monitor_plates");
  }
  if (mask & MON_VOLUME) {
    const MonVolArgs a{c.fld[EKPNP_RHO], c.fld[EKPNP_C], c.fld[EKPNP_CN], c.fld[EKPNP_T], c.fld[EKPNP_UX], c.fld[EKPNP_UY], c.fld[EKPNP_UZ],
                       (long long)c.plane, c.p.rho0, mask};
    hipLaunchKernelGGL(k_monitor_volume, dim3(nwg, c.nzl), dim3(MON_THREADS), 0, c.stream, a, m.vpart);
    note_launch(c, "k_monitor_volume");
  }
  if (mask & MON_VOLUME) {
    const int nitems = c.nzl * MON_NV;
    hipLaunchKernelGGL(k_monitor_planes, dim3((nitems + 63) / 64), dim3(64), 0, c.stream, m.vpart, nwg, nitems, m.vplane);
    note_launch(c, "k_monitor_planes");
  }
  const MonFinishArgs f{m.ppart, m.vpart, m.vplane, nb, nwg, c.nzl, has_top ? 1 : 0, has_bot ? 1 : 0, mask, c.p.K, c.p.dz,
                        to_ring ? (double*)m.ring.rows() : nullptr, (unsigned long long*)m.ring.alloc, m.ring.capacity, m.row};
  hipLaunchKernelGGL(k_monitor_finish, dim3(1), dim3(256), 0, c.stream, f);
  note_launch(c, "k_monitor_finish");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

namespace ekpnp {
int monitor_enqueue_row(Ctx& c) { return monitor_enqueue(c, c.mon->mask, true); }
void monitor_note_row(Ctx& c, int64_t step, double time) { ring_note_row(c.mon->ring, step, time); }
void monitor_count_steps(Ctx& c, int n) { c.mon->steps += n; }
void monitor_replayed_row(Ctx& c, double time) {
  ++c.mon->steps;
  monitor_note_row(c, c.mon->steps, time);
}
int monitor_step_done(Ctx& c) {
  if (!c.mon || !c.mon->ring.armed) return EKPNP_OK;
  MonState& m = *c.mon;
  ++m.steps;
  if (m.steps % m.every != 0) return EKPNP_OK;
  if (int rc = monitor_enqueue_row(c)) return rc;
  monitor_note_row(c, m.steps, c.t);
  return EKPNP_OK;
}
}  // namespace ekpnp

extern "C" const char* ekpnp_monitor_name(int id) { return id >= 0 && id < NM ? kMonitorNames[id] : nullptr; }

extern "C" int ekpnp_monitor_spec_check(const ekpnp_monitor_spec* spec) {
  std::string err;
  const int rc = monitor_check_spec(spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_monitor_sample(ekpnp_ctx* ctx, uint32_t quantities, double* out) {
  NEEDCTX(ctx);
  if (!out) return fail(c, "NULL pointer");
  if (quantities & ~MON_ALL) { c.err = "monitor: quantities = " + std::to_string(quantities) + " selects an id above " + std::to_string(NM - 1); return EKPNP_ERR_INVALID; }
  if (int rc = need_monitor(c)) return rc;
  if (int rc = monitor_enqueue(c, quantities ? quantities : MON_ALL, false)) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c.mon->row, NM * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_monitor_arm(ekpnp_ctx* ctx, const ekpnp_monitor_spec* spec) {
  NEEDCTX(ctx);
  if (int rc = monitor_check_spec(spec, c.err)) return rc;
  if (int rc = need_monitor(c)) return rc;
  MonState& m = *c.mon;
  drop_step_graph(c);  // a captured step holds (or lacks) the monitor's launches
  if (int rc = ring_arm(c, m.ring, spec->capacity, NM * sizeof(double), 16)) return rc;
  m.every = spec->every;
  m.mask = spec->quantities ? spec->quantities : MON_ALL;
  m.steps = 0;
  return EKPNP_OK;
}

extern "C" int ekpnp_monitor_disarm(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (c.mon && c.mon->ring.armed) {
    c.mon->ring.armed = false;  // the ring and its rows stay readable until the next arm
    drop_step_graph(c);
  }
  return EKPNP_OK;
}

extern "C" int ekpnp_monitor_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDCTX(ctx);
  if (!c.mon || !c.mon->ring.armed) return fail(c, "ekpnp_monitor_record: no monitor armed");
  if (int rc = monitor_enqueue_row(c)) return rc;
  monitor_note_row(c, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_monitor_count(const ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  if (!ctx) return EKPNP_ERR_INVALID;
  ring_count(ctx->c.mon ? &ctx->c.mon->ring : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_monitor_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, double* values) {
  NEEDCTX(ctx);
  return ring_read(c, c.mon ? &c.mon->ring : nullptr, "ekpnp_monitor_read", first, count, steps, times, values);
}

extern "C" int ekpnp_monitor_save(ekpnp_ctx* ctx, const char* path) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  int64_t rec = 0, dropped = 0;
  (void)ekpnp_monitor_count(ctx, &rec, &dropped);
  const int n = (int)(rec - dropped);
  std::vector<int64_t> steps((size_t)n);
  std::vector<double> times((size_t)n), values((size_t)n * NM);
  if (int rc = ekpnp_monitor_read(ctx, 0, n, steps.data(), times.data(), values.data())) return rc;
  return monitor_write_file(path, c.p, monitor_last_every(c), rec, dropped, n, steps.data(), times.data(), values.data(), c.err);
}
