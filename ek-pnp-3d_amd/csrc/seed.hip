// seed.hip — x-y patterns and reproducible white noise added to the field arrays on the device (include/ekpnp.h: ekpnp_seed,
// ekpnp_seed_host, ekpnp_seed_uniform, ekpnp_seed_spec_check; the reference's dead `perturb` branch, LBM.cu:646-661).
//
// ekpnp_initialization leaves every field uniform in x and y, so every node of a plane does the same arithmetic until rounding
// noise breaks the symmetry.  The only route to x-y structure used to be the host's: ekpnp_get_field, numpy, ekpnp_set_field -
// 1.07 GB per field each way at 512^3.  Here:
//   k_seed   grid (ceil(nx*ny / 256), interior planes of the context): one streaming read-modify-write pass over the selected
//            arrays; a lane takes one node of ALL selected fields (the tables are read once per node), Philox4x32-10 runs in
//            registers, indices are 64-bit, no LDS
// ekpnp_seed_host is THE definition, and the two agree bit for bit by construction: the tables (cos / sin of the host's <cmath>)
// are built by ONE host function and uploaded, the per-node arithmetic and the generator are ONE __host__ __device__ function
// each, and this object is built with -ffp-contract=off (csrc/Makefile, PINNED), so that neither side fuses a multiply-add.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "philox.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int SEED_THREADS = 256;
constexpr int SEED_MAXF = 7;                 // rho, c, cn, ux, uy, uz, T
constexpr uint32_t SEED_FIELDS = (1u << EKPNP_RHO) | (1u << EKPNP_C) | (1u << EKPNP_CN) | (1u << EKPNP_UX) | (1u << EKPNP_UY) | (1u << EKPNP_UZ) | (1u << EKPNP_T);

// (Philox4x32-10 and seed_uniform, the uniform number of (seed, global node, field): philox.h)

// the pattern at a node from the tables' values (include/ekpnp.h); every operation rounded once
__host__ __device__ inline double seed_pattern(int pattern, double cx, double sx, double cy, double sy, double c2y) {
  if (pattern == EKPNP_SEED_ROLLS) {
    const double a = cx * cy, b = sx * sy;
    return a - b;
  }
  if (pattern == EKPNP_SEED_SQUARES) return cx * cy;  // LBM.cu:651
  if (pattern == EKPNP_SEED_HEXAGONS) {               // LBM.cu:657
    const double a = cx * cy;
    const double b = 2.0 * a;
    const double d = b + c2y;
    return d / 3.0;
  }
  return 0.0;
}
// v of one field at a node: p = A*h; q = B*r; t = p + q; s = env*t; v = relative ? v + v*s : v + s
__host__ __device__ inline double seed_apply(double v, int relative, double A, double B, double h, double r, double env) {
  const double p = A * h;
  const double q = B * r;
  const double t = p + q;
  const double s = env * t;
  if (relative) {
    const double vs = v * s;
    return v + vs;
  }
  return v + s;
}

struct SeedArgs {
  double* f[SEED_MAXF];  // the selected arrays, [nzl][ny][nx]
  int id[SEED_MAXF];
  int nf;
  const double* cX;      // [nx]
  const double* sX;
  const double* cY;      // [ny]
  const double* sY;
  const double* c2Y;
  const double* env;     // [nzl], by local plane
  int nx, zl0, z0;       // first interior local plane of the launch, global index of local plane 0
  long long plane;
  int pattern, relative;
  double A, B;
  uint64_t seed;
};

__global__ void __launch_bounds__(SEED_THREADS) k_seed(SeedArgs a) {
  const long long i = (long long)blockIdx.x * SEED_THREADS + threadIdx.x;  // node of the plane
  if (i >= a.plane) return;
  const int zl = a.zl0 + (int)blockIdx.y;
  const long long y = i / a.nx, x = i - y * a.nx;
  const double h = seed_pattern(a.pattern, a.cX[x], a.sX[x], a.cY[y], a.sY[y], a.c2Y[y]);
  const double env = a.env[zl];
  const uint64_t node = (uint64_t)((long long)(a.z0 + zl) * a.plane + i);
  const long long t = (long long)zl * a.plane + i;
#pragma unroll
  for (int k = 0; k < SEED_MAXF; ++k) {
    if (k < a.nf) {
      const double r = seed_uniform(a.seed, node, a.id[k]);
      a.f[k][t] = seed_apply(a.f[k][t], a.relative, a.A, a.B, h, r, env);
    }
  }
}

// The tables of planes z0 .. z0 + nzl - 1, [cX | sX | cY | sY | c2Y | env]: 2 nx + 3 ny + nzl doubles.  64-bit products,
// non-negative remainders, the host's <cmath>.
static void seed_tables(const ekpnp_params& p, const ekpnp_seed_spec& s, int z0, int nzl, double* t) {
  const long long nx = p.nx, ny = p.ny;
  auto rem = [](long long a, long long n) { const long long r = a % n; return r < 0 ? r + n : r; };
  double *cX = t, *sX = cX + nx, *cY = sX + nx, *sY = cY + ny, *c2Y = sY + ny, *env = c2Y + ny;
  for (long long x = 0; x < nx; ++x) {
    const double th = 2.0 * M_PI * (double)rem((long long)s.mx * x, nx) / (double)nx;
    cX[x] = std::cos(th);
    sX[x] = std::sin(th);
  }
  for (long long y = 0; y < ny; ++y) {
    const double th = 2.0 * M_PI * (double)rem((long long)s.my * y, ny) / (double)ny;
    cY[y] = std::cos(th);
    sY[y] = std::sin(th);
    c2Y[y] = std::cos(2.0 * M_PI * (double)rem(2LL * s.my * y, ny) / (double)ny);
  }
  for (int z = 0; z < nzl; ++z) env[z] = std::sin(M_PI * (double)(z0 + z) / (double)(p.nz - 1));
}
static inline size_t seed_table_doubles(const ekpnp_params& p, int nzl) { return 2 * (size_t)p.nx + 3 * (size_t)p.ny + (size_t)nzl; }

int seed_check_spec(const ekpnp_params& p, const ekpnp_seed_spec* s, std::string& err) {
  char num[64];
  if (!s) { err = "seed: NULL spec"; return EKPNP_ERR_INVALID; }
  if (p.nx < 1 || p.ny < 1) { err = "seed: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (p.nz < 3) { err = "seed: nz = " + std::to_string(p.nz) + " (must be >= 3: there is no interior plane)"; return EKPNP_ERR_INVALID; }
  if (s->fields == 0) { err = "seed: fields = 0 selects no field"; return EKPNP_ERR_INVALID; }
  if (s->fields & ~SEED_FIELDS) {
    err = "seed: fields = " + std::to_string(s->fields) + " selects phi, Ex, Ey or Ez or an id above 10 (only rho, c, cn, ux, uy, uz, T are seeded)";
    return EKPNP_ERR_INVALID;
  }
  if (s->pattern < 0 || s->pattern > 3) { err = "seed: pattern = " + std::to_string(s->pattern) + " (must be 0 .. 3)"; return EKPNP_ERR_INVALID; }
  if (s->mx < 0 || s->mx > p.nx / 2) { err = "seed: mx = " + std::to_string(s->mx) + " outside 0 .. " + std::to_string(p.nx / 2); return EKPNP_ERR_INVALID; }
  if (s->my < -(p.ny / 2) || s->my > p.ny / 2) {
    err = "seed: my = " + std::to_string(s->my) + " outside " + std::to_string(-(p.ny / 2)) + " .. " + std::to_string(p.ny / 2);
    return EKPNP_ERR_INVALID;
  }
  if (s->pattern == EKPNP_SEED_HEXAGONS && 2LL * std::llabs((long long)s->my) > p.ny / 2) {
    err = "seed: hexagons with my = " + std::to_string(s->my) + ": |2*my| exceeds ny/2 = " + std::to_string(p.ny / 2);
    return EKPNP_ERR_INVALID;
  }
  if (s->relative < 0 || s->relative > 1) { err = "seed: relative = " + std::to_string(s->relative) + " (must be 0 or 1)"; return EKPNP_ERR_INVALID; }
  if (s->reserved != 0) { err = "seed: reserved = " + std::to_string(s->reserved) + " (must be 0)"; return EKPNP_ERR_INVALID; }
  if (!std::isfinite(s->amplitude)) { std::snprintf(num, sizeof num, "%g", s->amplitude); err = std::string("seed: amplitude = ") + num + " is not finite"; return EKPNP_ERR_INVALID; }
  if (!std::isfinite(s->noise)) { std::snprintf(num, sizeof num, "%g", s->noise); err = std::string("seed: noise = ") + num + " is not finite"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

// one device buffer and its pinned host twin, sized once per context; `landed` marks the last upload (the host twin is reused)
struct SeedState {
  double* dev = nullptr;
  double* host = nullptr;
  hipEvent_t landed = nullptr;
  size_t bytes = 0;
};

void seed_release(Ctx& c) {
  if (!c.seed) return;
  if (c.seed->landed) (void)hipEventDestroy(c.seed->landed);
  if (c.seed->dev) (void)hipFree(c.seed->dev);
  if (c.seed->host) (void)hipHostFree(c.seed->host);
  delete c.seed;
  c.seed = nullptr;
}

}  // namespace ekpnp

extern "C" int ekpnp_seed_spec_check(const ekpnp_params* p, const ekpnp_seed_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "seed: NULL parameters";
  else rc = seed_check_spec(*p, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" double ekpnp_seed_uniform(uint64_t seed, uint64_t node, int field_id) { return seed_uniform(seed, node, field_id); }

extern "C" int ekpnp_seed_host(const ekpnp_params* p, const ekpnp_seed_spec* spec, int field_id, int z0, int nz_local, double* planes) {
  if (int rc = ekpnp_seed_spec_check(p, spec)) return rc;
  if (!planes) { set_create_error("seed: NULL pointer"); return EKPNP_ERR_INVALID; }
  if (field_id < 0 || field_id >= EKPNP_NFIELDS) { set_create_error("seed: field_id = " + std::to_string(field_id) + " outside 0 .. 10"); return EKPNP_ERR_INVALID; }
  if (z0 < 0 || nz_local < 0 || (long long)z0 + nz_local > p->nz) {
    set_create_error("seed: planes " + std::to_string(z0) + " .. " + std::to_string((long long)z0 + nz_local - 1) + " are not inside nz = " + std::to_string(p->nz));
    return EKPNP_ERR_INVALID;
  }
  std::vector<double> tab(seed_table_doubles(*p, nz_local));
  seed_tables(*p, *spec, z0, nz_local, tab.data());
  const long long nx = p->nx, ny = p->ny, plane = nx * ny;
  const double *cX = tab.data(), *sX = cX + nx, *cY = sX + nx, *sY = cY + ny, *c2Y = sY + ny, *env = c2Y + ny;
  for (int zl = 0; zl < nz_local; ++zl) {
    const int z = z0 + zl;
    if (z < 1 || z > p->nz - 2) continue;  // the plates keep their boundary values
    for (long long y = 0; y < ny; ++y)
      for (long long x = 0; x < nx; ++x) {
        const long long i = y * nx + x;
        const double h = seed_pattern(spec->pattern, cX[x], sX[x], cY[y], sY[y], c2Y[y]);
        const double r = seed_uniform(spec->seed, (uint64_t)((long long)z * plane + i), field_id);
        double& v = planes[(long long)zl * plane + i];
        v = seed_apply(v, spec->relative, spec->amplitude, spec->noise, h, r, env[zl]);
      }
  }
  return EKPNP_OK;
}

extern "C" int ekpnp_seed(ekpnp_ctx* ctx, const ekpnp_seed_spec* spec) {
  NEEDCTX(ctx);
  if (int rc = seed_check_spec(c.p, spec, c.err)) return rc;
  if (c.nzl > 65535) { c.err = "seed: more than 65535 planes in one context"; return EKPNP_ERR_INVALID; }
  const size_t bytes = seed_table_doubles(c.p, c.nzl) * sizeof(double);
  if (!c.seed) {
    SeedState* s = new (std::nothrow) SeedState();
    if (!s) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
    c.seed = s;  // (whatever the calls below leave behind is freed by ekpnp_destroy)
    HIPCHK(c, hipMalloc((void**)&s->dev, bytes));
    s->bytes = bytes;
    c.bytes += bytes;
    HIPCHK(c, hipHostMalloc((void**)&s->host, bytes, hipHostMallocDefault));
    HIPCHK(c, hipEventCreateWithFlags(&s->landed, hipEventDisableTiming));
  } else if (!c.seed->dev || !c.seed->host || !c.seed->landed) {
    c.err = "seed: the table buffer could not be made earlier";
    return EKPNP_ERR_HIP;
  } else {
    HIPCHK(c, hipEventSynchronize(c.seed->landed));  // the previous seed's upload has left the pinned twin (not a wait for the stream)
  }
  SeedState& s = *c.seed;
  seed_tables(c.p, *spec, c.z0, c.nzl, s.host);
  HIPCHK(c, hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, c.stream));
  HIPCHK(c, hipEventRecord(s.landed, c.stream));
  // the interior planes this context holds
  const int zl0 = c.z0 == 0 ? 1 : 0, zl1 = c.z0 + c.nzl == c.p.nz ? c.nzl - 1 : c.nzl;
  c.rhs_ready = false;  // c, cn may have changed: the next solve re-reads them
  if (zl1 <= zl0) return EKPNP_OK;
  SeedArgs a{};
  a.nf = 0;
  for (int id = 0; id < EKPNP_NFIELDS; ++id)
    if (spec->fields & (1u << id)) {
      a.f[a.nf] = c.fld[id];
      a.id[a.nf] = id;
      ++a.nf;
    }
  const size_t nx = (size_t)c.p.nx, ny = (size_t)c.p.ny;
  a.cX = s.dev;
  a.sX = a.cX + nx;
  a.cY = a.sX + nx;
  a.sY = a.cY + ny;
  a.c2Y = a.sY + ny;
  a.env = a.c2Y + ny;
  a.nx = c.p.nx;
  a.zl0 = zl0;
  a.z0 = c.z0;
  a.plane = (long long)c.plane;
  a.pattern = spec->pattern;
  a.relative = spec->relative;
  a.A = spec->amplitude;
  a.B = spec->noise;
  a.seed = spec->seed;
  const unsigned gx = (unsigned)((c.plane + SEED_THREADS - 1) / SEED_THREADS);
  hipLaunchKernelGGL(k_seed, dim3(gx, (unsigned)(zl1 - zl0)), dim3(SEED_THREADS), 0, c.stream, a);
  note_launch(c, "k_seed");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}
