// modes.hip — projection of a field onto chosen x-y Fourier modes, per z plane, and its time series (include/ekpnp.h:
// ekpnp_mode_amplitudes, ekpnp_modes_*; no reference counterpart).
//
// What is plotted first of a seeded pattern (seed.hip) is the amplitude of its Fourier mode against time.  A projection onto
// at most EKPNP_MAX_MODES chosen modes needs no transform: it is one more fixed-order plane reduction of the kind stats.hip has.
//   k_mode_partials<NM,ROW64>  grid (ceil(nx*ny / MODE_CHUNK), nzl), the shape of stats.hip's k_plane_partials: a workgroup reads
//                        MODE_CHUNK consecutive nodes of ONE plane of ONE array once (8 B per node whatever the number of modes)
//                        and stores, per mode, its partial sums of v cos(theta) and v sin(theta);
//                        cos(theta) = cX*cY - sX*sY, sin(theta) = sX*cY + cX*sY from the per-mode tables, which the lanes read
//                        as (cos, sin) pairs through the caches (at most 16 (nx + ny) pairs: they stay in L2)
//   k_mode_finish        one workgroup per plane: the partial sums in ascending workgroup order -> (a, b) [mode][plane]
//   k_mode_energy        one lane per mode: E = sum_z (a^2 + b^2) in ascending z, as e = a*a; e = e + b*b; E = E + e, into the
//                        ring slot the host names (record is an explicit enqueue, so the host knows the slot: no device cursor)
// No atomics.  Thread t of workgroup b takes nodes b*MODE_CHUNK + k*256 + t, k ascending; fixed trees over lanes and waves; partial
// sums in ascending b: the order depends on nx*ny alone, not on z0, nzl, the buffer mode or the device.  The object is built with
// -ffp-contract=off (csrc/Makefile, PINNED) and the hot loop spells its fused multiply-adds out, so every instantiation of the
// template rounds a mode's terms the same way: (a, b) do not depend on how many modes are projected beside it.
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "reduce.h"
#include "ring.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int MODE_THREADS = 256;
constexpr int MODE_PER_THREAD = 16;
constexpr int MODE_CHUNK = MODE_THREADS * MODE_PER_THREAD;  // nodes of a plane per workgroup (stats.hip's STATS_CHUNK)
constexpr int MAXM = EKPNP_MAX_MODES;

static const char* const kFieldNames[EKPNP_NFIELDS] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"};

struct ModeArgs {
  const double* v;      // [nzl][ny][nx]
  const double2* tX;    // [NM][nx]: (cos, sin) of 2 pi ((m x) mod nx) / nx
  const double2* tY;    // [NM][ny]: (cos, sin) of 2 pi ((n y) mod ny) / ny
  long long plane;
  int nx, ny;
  int dx, dy;           // MODE_THREADS = dy * nx + dx: how (x, y) move from one node of a thread to its next
};

// partial[((z * nwg + b) * NM + j) * 2 + {0: cos, 1: sin}]
// A thread first loads its MODE_PER_THREAD values (independent loads, all in flight), then takes the modes one after the other over
// them - k ascending within a mode, which is all the order of additions asks for.  ROW64: nx is a multiple of 64, so the 64
// consecutive nodes of a wavefront lie in one row and the row's (cos, sin) pair is ONE wave-uniform (scalar) load instead of 64
// identical ones; either way the same two numbers reach every lane.
template <int NM, bool ROW64>
__global__ void __launch_bounds__(MODE_THREADS) k_mode_partials(ModeArgs a, double* __restrict__ partial) {
  __shared__ double lds[2 * NM][MODE_THREADS / 64];
  const long long first = (long long)blockIdx.x * MODE_CHUNK + threadIdx.x;
  const double* __restrict__ v = a.v + (long long)blockIdx.y * a.plane;
  const double2* __restrict__ tXp = a.tX;
  const double2* __restrict__ tYp = a.tY;
  double val[MODE_PER_THREAD];
  int xs[MODE_PER_THREAD], ys[MODE_PER_THREAD];
  unsigned inside = 0;
  {
    const long long y0 = first / a.nx;
    int x = (int)(first - y0 * a.nx), y = (int)y0;
#pragma unroll
    for (int k = 0; k < MODE_PER_THREAD; ++k) {
      const long long i = first + (long long)k * MODE_THREADS;
      const bool in = i < a.plane;
      val[k] = in ? v[i] : 0.0;
      if (in) inside |= 1u << k;
      xs[k] = in ? x : 0;  // (a lane beyond the plane reads entry 0 of the tables and adds nothing)
      ys[k] = in ? y : 0;  // (ROW64: the plane is a multiple of 64 nodes too, a wavefront is inside or outside as a whole)
      x += a.dx;
      y += a.dy;
      if (x >= a.nx) { x -= a.nx; ++y; }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    const double2* __restrict__ tx = tXp + (long long)j * a.nx;
    const double2* __restrict__ ty = tYp + (long long)j * a.ny;
    double sc = 0.0, ss = 0.0;
#pragma unroll
    for (int k = 0; k < MODE_PER_THREAD; ++k) {
      const double2 cx = tx[xs[k]];
      const double2 cy = ty[ROW64 ? __builtin_amdgcn_readfirstlane(ys[k]) : ys[k]];
      if (inside & (1u << k)) {
        const double ct = __builtin_fma(cx.x, cy.x, -(cx.y * cy.y));  // cX*cY - sX*sY
        const double st = __builtin_fma(cx.y, cy.x, cx.x * cy.y);     // sX*cY + cX*sY
        sc = __builtin_fma(val[k], ct, sc);
        ss = __builtin_fma(val[k], st, ss);
      }
    }
    const double rc = wave_sum(sc), rs = wave_sum(ss);
    if (lane == 0) { lds[2 * j][wave] = rc; lds[2 * j + 1][wave] = rs; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * NM) {
    double r = lds[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < MODE_THREADS / 64; ++w) r += lds[threadIdx.x][w];
    partial[((long long)blockIdx.y * gridDim.x + blockIdx.x) * (2 * NM) + threadIdx.x] = r;
  }
}

// out[(j * nzl + z) * 2 + ab] = the plane's partial sums in ascending workgroup order (only the nm modes asked for); sixteen loads
// in flight, as in monitor.hip's k_monitor_planes: the chain of additions is short, the latency of a load is not
__global__ void __launch_bounds__(64) k_mode_finish(const double* __restrict__ partial, int nwg, int nzl, int NM, int nm, double* __restrict__ out) {
  const int z = blockIdx.x, q = threadIdx.x;
  if (q >= 2 * nm) return;
  const double* p = partial + (long long)z * nwg * (2 * NM) + q;
  double r = 0.0;
  for (int b0 = 0; b0 < nwg; b0 += 16) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = b0 + k < nwg ? p[(long long)(b0 + k) * (2 * NM)] : 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (b0 + k < nwg) r += v[k];
  }
  out[((long long)(q >> 1) * nzl + z) * 2 + (q & 1)] = r;
}

// row[j] = sum over the context's planes in ascending z of a^2 + b^2; every operation rounded once (eight planes' loads in flight)
__global__ void __launch_bounds__(64) k_mode_energy(const double* __restrict__ ab, int nzl, int nm, double* __restrict__ row) {
  const int j = threadIdx.x;
  if (j >= nm) return;
  const double2* p = (const double2*)ab + (long long)j * nzl;
  double E = 0.0;
  for (int z0 = 0; z0 < nzl; z0 += 8) {
    double2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = z0 + k < nzl ? p[z0 + k] : double2{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (z0 + k < nzl) {
        double e = v[k].x * v[k].x;
        const double bb = v[k].y * v[k].y;
        e = e + bb;
        E = E + e;
      }
  }
  row[j] = E;
}

// Host side of a context's mode projection: made by the first ekpnp_mode_amplitudes / ekpnp_modes_arm, never by a context that uses neither.
struct ModeState {
  double* scratch = nullptr;  // one allocation: [partials | (a, b) of the last pass | tables of the armed spec | tables of a synchronous call]
  size_t scratch_bytes = 0;
  double* part = nullptr;
  double* ab = nullptr;
  double2* tab_armed = nullptr;
  double2* tab_sync = nullptr;
  Ring ring;                  // rows of [nmodes] doubles
  ekpnp_modes_spec spec{};
  std::vector<double2> host_tab;  // what the last arm uploaded (kept while the copy may be in flight)
};

static inline int mode_workgroups(const Ctx& c) { return (int)(((long long)c.plane + MODE_CHUNK - 1) / MODE_CHUNK); }
static inline size_t mode_table_pairs(const Ctx& c) { return (size_t)MAXM * ((size_t)c.p.nx + (size_t)c.p.ny); }
static inline int mode_template(int nm) { return nm <= 1 ? 1 : nm <= 2 ? 2 : nm <= 4 ? 4 : nm <= 8 ? 8 : 16; }

int modes_check_spec(const ekpnp_params& p, const ekpnp_modes_spec* s, std::string& err) {
  if (!s) { err = "modes: NULL spec"; return EKPNP_ERR_INVALID; }
  if (p.nx < 1 || p.ny < 1) { err = "modes: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (s->field_id < 0 || s->field_id >= EKPNP_NFIELDS) { err = "modes: field_id = " + std::to_string(s->field_id) + " outside 0 .. 10"; return EKPNP_ERR_INVALID; }
  if (s->nmodes < 1 || s->nmodes > MAXM) { err = "modes: nmodes = " + std::to_string(s->nmodes) + " outside 1 .. " + std::to_string(MAXM); return EKPNP_ERR_INVALID; }
  for (int j = 0; j < s->nmodes; ++j) {
    if (s->m[j] < 0 || s->m[j] > p.nx / 2) {
      err = "modes: m[" + std::to_string(j) + "] = " + std::to_string(s->m[j]) + " outside 0 .. " + std::to_string(p.nx / 2);
      return EKPNP_ERR_INVALID;
    }
    if (s->n[j] < -((p.ny - 1) / 2) || s->n[j] > p.ny / 2) {
      err = "modes: n[" + std::to_string(j) + "] = " + std::to_string(s->n[j]) + " outside " + std::to_string(-((p.ny - 1) / 2)) + " .. " + std::to_string(p.ny / 2);
      return EKPNP_ERR_INVALID;
    }
  }
  return EKPNP_OK;
}

// [NM][nx] then [NM][ny] pairs, the expressions of the seed's tables; the modes beyond nmodes project onto nothing (zeros)
static void mode_tables(const ekpnp_params& p, const ekpnp_modes_spec& s, int NM, std::vector<double2>& t) {
  const long long nx = p.nx, ny = p.ny;
  auto rem = [](long long a, long long n) { const long long r = a % n; return r < 0 ? r + n : r; };
  t.assign((size_t)NM * (size_t)(nx + ny), double2{0.0, 0.0});
  double2* tX = t.data();
  double2* tY = tX + (size_t)NM * nx;
  for (int j = 0; j < s.nmodes; ++j) {
    for (long long x = 0; x < nx; ++x) {
      const double th = 2.0 * M_PI * (double)rem((long long)s.m[j] * x, nx) / (double)nx;
      tX[(size_t)j * nx + x] = double2{std::cos(th), std::sin(th)};
    }
    for (long long y = 0; y < ny; ++y) {
      const double th = 2.0 * M_PI * (double)rem((long long)s.n[j] * y, ny) / (double)ny;
      tY[(size_t)j * ny + y] = double2{std::cos(th), std::sin(th)};
    }
  }
}

const ekpnp_modes_spec* modes_armed_spec(const Ctx& c) { return c.modes && c.modes->ring.ever_armed ? &c.modes->spec : nullptr; }

bool modes_armed(const Ctx& c) { return c.modes && c.modes->ring.armed; }

void modes_release(Ctx& c) {
  if (!c.modes) return;
  if (c.modes->scratch) (void)hipFree(c.modes->scratch);
  ring_release(c.modes->ring);
  delete c.modes;
  c.modes = nullptr;
}

int modes_write_file(const char* path, const ekpnp_params& p, const ekpnp_modes_spec& spec, int64_t recorded, int64_t dropped, int n,
                     const int64_t* steps, const double* times, const double* values, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open modes file"; return EKPNP_ERR_INVALID; }
  std::fprintf(f, "# ekpnp modes nx %d ny %d nz %d field %s recorded %lld dropped %lld\n", p.nx, p.ny, p.nz, kFieldNames[spec.field_id], (long long)recorded,
               (long long)dropped);
  std::fprintf(f, "# step time");
  for (int j = 0; j < spec.nmodes; ++j) std::fprintf(f, " E_%d_%d", spec.m[j], spec.n[j]);
  std::fprintf(f, "\n");
  for (int r = 0; r < n; ++r) {
    std::fprintf(f, "%lld %.17g", (long long)steps[r], times[r]);
    for (int j = 0; j < spec.nmodes; ++j) std::fprintf(f, " %.17g", values[(size_t)r * spec.nmodes + j]);
    std::fprintf(f, "\n");
  }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on modes file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

}  // namespace ekpnp

// the host state, the reduction scratch and the two table slots, once
static int need_modes(Ctx& c) {
  if (c.modes) return EKPNP_OK;
  if (c.nzl > 65535) return fail(c, "modes: more than 65535 planes in one context");
  ModeState* m = new (std::nothrow) ModeState();
  if (!m) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  const size_t npart = (size_t)c.nzl * (size_t)mode_workgroups(c) * 2 * MAXM, nab = (size_t)MAXM * (size_t)c.nzl * 2, ntab = 2 * mode_table_pairs(c);
  m->scratch_bytes = (npart + nab + 2 * ntab) * sizeof(double);
  const hipError_t e = hipMalloc((void**)&m->scratch, m->scratch_bytes);
  if (e != hipSuccess) {
    delete m;
    HIPCHK(c, e);
  }
  m->part = m->scratch;
  m->ab = m->part + npart;
  m->tab_armed = (double2*)(m->ab + nab);  // (npart and nab are even: the pairs are 16-byte aligned)
  m->tab_sync = m->tab_armed + mode_table_pairs(c);
  c.bytes += m->scratch_bytes;
  c.modes = m;
  return EKPNP_OK;
}

// enqueue the projection of the current field onto the modes of `spec` (tables already on the device at `tab`) into ModeState::ab
static int modes_enqueue(Ctx& c, const ekpnp_modes_spec& spec, const double2* tab) {
  ModeState& m = *c.modes;
  const int id = spec.field_id;
  if (id == EKPNP_PHI || id == EKPNP_EX || id == EKPNP_EY || id == EKPNP_EZ) {
    if (int rc = ensure_efield(c)) return rc;  // the arrays as ekpnp_get_field would return them
  }
  const int NM = mode_template(spec.nmodes), nwg = mode_workgroups(c);
  const ModeArgs a{c.fld[id], tab, tab + (size_t)NM * c.p.nx, (long long)c.plane, c.p.nx, c.p.ny, MODE_THREADS % c.p.nx, MODE_THREADS / c.p.nx};
  const dim3 grid(nwg, c.nzl), block(MODE_THREADS);
  const bool row64 = c.p.nx % 64 == 0;
#define MODE_LAUNCH(N)                                                                                              \
  case N:                                                                                                                 \
    if (row64) hipLaunchKernelGGL((k_mode_partials<N, true>), grid, block, 0, c.stream, a, m.part);                       \
    else hipLaunchKernelGGL((k_mode_partials<N, false>), grid, block, 0, c.stream, a, m.part);                            \
    break
  switch (NM) {
    MODE_LAUNCH(1);
    MODE_LAUNCH(2);
    MODE_LAUNCH(4);
    MODE_LAUNCH(8);
    default:
    MODE_LAUNCH(16);
  }
#undef MODE_LAUNCH
  note_launch(c, "k_mode_partials");
  hipLaunchKernelGGL(k_mode_finish, dim3(c.nzl), dim3(64), 0, c.stream, m.part, nwg, c.nzl, NM, spec.nmodes, m.ab);
  note_launch(c, "k_mode_finish");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_modes_spec_check(const ekpnp_params* p, const ekpnp_modes_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "modes: NULL parameters";
  else rc = modes_check_spec(*p, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_mode_amplitudes(ekpnp_ctx* ctx, const ekpnp_modes_spec* spec, double* host_out) {
  NEEDCTX(ctx);
  if (!host_out) return fail(c, "NULL pointer");
  if (int rc = modes_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = need_modes(c)) return rc;
  ModeState& m = *c.modes;
  std::vector<double2> tab;
  mode_tables(c.p, *spec, mode_template(spec->nmodes), tab);
  HIPCHK(c, hipMemcpyAsync(m.tab_sync, tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice, c.stream));
  int rc = modes_enqueue(c, *spec, m.tab_sync);
  if (rc == EKPNP_OK) {
    const hipError_t e = hipMemcpyAsync(host_out, m.ab, (size_t)spec->nmodes * c.nzl * 2 * sizeof(double), hipMemcpyDeviceToHost, c.stream);
    if (e != hipSuccess) { c.err = std::string("hipMemcpyAsync: ") + hipGetErrorString(e); rc = EKPNP_ERR_HIP; }
  }
  HIPCHK(c, hipStreamSynchronize(c.stream));  // (also before `tab` goes away)
  return rc;
}

extern "C" int ekpnp_modes_arm(ekpnp_ctx* ctx, const ekpnp_modes_spec* spec, int capacity) {
  NEEDCTX(ctx);
  if (int rc = modes_check_spec(c.p, spec, c.err)) return rc;
  if (capacity < 1) { c.err = "modes: capacity = " + std::to_string(capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (int rc = need_modes(c)) return rc;
  ModeState& m = *c.modes;
  m.ring.armed = false;
  HIPCHK(c, hipStreamSynchronize(c.stream));  // rows of an earlier arm may still be on their way through the tables
  mode_tables(c.p, *spec, mode_template(spec->nmodes), m.host_tab);
  HIPCHK(c, hipMemcpyAsync(m.tab_armed, m.host_tab.data(), m.host_tab.size() * sizeof(double2), hipMemcpyHostToDevice, c.stream));
  m.spec = *spec;
  return ring_arm(c, m.ring, capacity, (size_t)spec->nmodes * sizeof(double));
}

extern "C" int ekpnp_modes_disarm(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (c.modes) c.modes->ring.armed = false;  // the ring and its rows stay readable until the next arm
  return EKPNP_OK;
}

extern "C" int ekpnp_modes_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDCTX(ctx);
  if (!c.modes || !c.modes->ring.armed) return fail(c, "ekpnp_modes_record: no mode tracking armed");
  ModeState& m = *c.modes;
  if (int rc = modes_enqueue(c, m.spec, m.tab_armed)) return rc;
  hipLaunchKernelGGL(k_mode_energy, dim3(1), dim3(64), 0, c.stream, m.ab, c.nzl, m.spec.nmodes, (double*)ring_next_row(m.ring));
  note_launch(c, "k_mode_energy");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  ring_note_row(m.ring, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_modes_count(const ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  if (!ctx) return EKPNP_ERR_INVALID;
  ring_count(ctx->c.modes ? &ctx->c.modes->ring : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_modes_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, double* values) {
  NEEDCTX(ctx);
  return ring_read(c, c.modes ? &c.modes->ring : nullptr, "ekpnp_modes_read", first, count, steps, times, values);
}

extern "C" int ekpnp_modes_save(ekpnp_ctx* ctx, const char* path) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  const ekpnp_modes_spec* spec = modes_armed_spec(c);
  if (!spec) return fail(c, "ekpnp_modes_save: no mode tracking was armed");
  int64_t rec = 0, dropped = 0;
  (void)ekpnp_modes_count(ctx, &rec, &dropped);
  const int n = (int)(rec - dropped);
  std::vector<int64_t> steps((size_t)n);
  std::vector<double> times((size_t)n), values((size_t)n * spec->nmodes);
  if (int rc = ekpnp_modes_read(ctx, 0, n, steps.data(), times.data(), values.data())) return rc;
  return modes_write_file(path, c.p, *spec, rec, dropped, n, steps.data(), times.data(), values.data(), c.err);
}
