// snapshot.hip — coarsened FP32 snapshots of the fields, written while the run continues (include/ekpnp.h: ekpnp_snapshot_*;
// no reference counterpart).
//
// A picture of the vortices (LBM.cu:646-661 are the cells its users study) used to cost one ekpnp_get_field per field - 1.07 GB
// of FP64 each at 512^3, through pageable memory, with the stream waiting - or a %10.6f text row per node.  Here:
//   k_snapshot   ONE launch per snapshot over the selected fields (pointers by value, as StatsFields): one thread per output
//                node of one field.  z is SAMPLED (output plane k is global plane k*cz: skipped planes are never read), x and y
//                are block means: the lane reads cx contiguous doubles from each of cy rows and adds them one at a time,
//                yy ascending outside, xx ascending inside, S = S + v in FP64; the result is (float)(S / (cx*cy)).  No tree, no
//                shuffle, no atomic: the bits depend on the field values alone.  Lane l of a wave takes output x0 + l of one
//                output row, so a wave reads 64*cx*8 contiguous bytes per input row and writes 256 contiguous bytes.
//   pipeline     two device staging slots, two pinned host buffers, one side stream, made on first use.  begin: the compute
//                stream waits for the slot's previous copy, runs the kernel, records an event; the side stream waits for it,
//                copies to the pinned buffer and records "landed".  finish waits for "landed" only - never for the compute
//                stream - and writes the legacy VTK file on the calling thread while ekpnp_step keeps the device busy.
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "ekpnp_internal.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int SNAP_LANES = 64;  // outputs of one row per wave
constexpr int SNAP_ROWS = 4;    // output rows (waves) per workgroup

struct SnapFields {
  const double* f[EKPNP_NFIELDS];
  unsigned aligned16;  // bit i: f[i] is 16-byte aligned (a caller-bound array may be 8-byte aligned only)
};

struct SnapGeom {
  long long nx, plane;  // doubles per input row / plane
  int X, Y;             // output row length and rows per plane
  int cz;
  int swap;             // store the float byte-swapped (the file path)
  int zl_first;         // local plane of the first sampled output plane
  int xchunks;          // ceil(X / SNAP_LANES): blockIdx.x = field slot * xchunks + chunk
  double inv;           // 1 / (cx*cy), a power of two: S * inv is S / (cx*cy) bit for bit
};

// 8-byte load that stays one: a wavefront-scope relaxed atomic load is a plain global_load_dwordx2 that the compiler may not
// merge with its neighbour into a 16-byte access (it does merge ordinary loads, whatever the alignment)
__device__ __forceinline__ double snap_load8(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// grid (nfields * xchunks, ceil(Y / SNAP_ROWS), sampled planes of this context), block (SNAP_LANES, SNAP_ROWS); instantiated per
// (cx, cy): both loops unroll, the cx*cy loads of a node are in flight together and the additions follow in the fixed order
template <int CX, int CY>
__global__ void __launch_bounds__(SNAP_LANES* SNAP_ROWS) k_snapshot(SnapFields a, SnapGeom g, float* __restrict__ out) {
  const int slot = (int)blockIdx.x / g.xchunks;
  const int chunk = (int)blockIdx.x - slot * g.xchunks;
  const int x = chunk * SNAP_LANES + (int)threadIdx.x;
  const int y = (int)blockIdx.y * SNAP_ROWS + (int)threadIdx.y;
  const int k = (int)blockIdx.z;
  if (x >= g.X || y >= g.Y) return;
  const double* __restrict__ src =
      a.f[slot] + ((long long)g.zl_first + (long long)k * g.cz) * g.plane + (long long)y * CY * g.nx + (long long)x * CX;
  double v[CY][CX];
  if (CX >= 2 && ((a.aligned16 >> slot) & 1u)) {  // nx and x*CX are even then: every row start is as aligned as the array
#pragma unroll
    for (int yy = 0; yy < CY; ++yy)
#pragma unroll
      for (int xx = 0; xx < CX / 2; ++xx) {
        const double2 w = reinterpret_cast<const double2*>(src + (long long)yy * g.nx)[xx];
        v[yy][2 * xx] = w.x;
        v[yy][(2 * xx + 1) % CX] = w.y;
      }
  } else {
#pragma unroll
    for (int yy = 0; yy < CY; ++yy)
#pragma unroll
      for (int xx = 0; xx < CX; ++xx) v[yy][xx] = snap_load8(src + (long long)yy * g.nx + xx);
  }
  double S = v[0][0];
#pragma unroll
  for (int yy = 0; yy < CY; ++yy)
#pragma unroll
    for (int xx = 0; xx < CX; ++xx)
      if (yy | xx) S = S + v[yy][xx];
  const float r = (float)(S * g.inv);
  const long long o = (((long long)slot * gridDim.z + k) * g.Y + y) * g.X + x;
  if (g.swap) reinterpret_cast<unsigned*>(out)[o] = __builtin_bswap32(__float_as_uint(r));  // legacy VTK binary is big-endian
  else out[o] = r;
}

struct SnapSlot {
  float* dev = nullptr;
  float* host = nullptr;  // pinned
  size_t cap = 0;         // bytes of each
  hipEvent_t done = nullptr, landed = nullptr;  // kernel finished (compute stream) / copy finished (side stream)
  bool used = false;      // `landed` has been recorded at least once
};

struct SnapPending {
  int slot = 0;
  ekpnp_snapshot_spec spec{};
  unsigned mask = 0;      // fields, never 0
  int nf = 0, k0 = 0, kn = 0;  // selected fields, first output plane of this context and how many it holds
  size_t bytes = 0;
  bool to_file = false;
  std::string path;
  double time = 0.0;
};

struct SnapState {
  SnapSlot slot[2];
  hipStream_t side = nullptr;
  int next = 0;
  std::deque<SnapPending> q;
};

static const char* const kSnapNames[EKPNP_NFIELDS] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"};
constexpr unsigned SNAP_ALL = (1u << EKPNP_NFIELDS) - 1u;

static inline int popcount(unsigned m) { return __builtin_popcount(m); }

int snapshot_check_spec(const ekpnp_params& p, const ekpnp_snapshot_spec* s, std::string& err) {
  if (!s) { err = "snapshot: NULL spec"; return EKPNP_ERR_INVALID; }
  if (s->fields & ~SNAP_ALL) {
    err = "snapshot: field mask " + std::to_string(s->fields) + " has bits above field " + std::to_string(EKPNP_NFIELDS - 1);
    return EKPNP_ERR_INVALID;
  }
  const int cxy[2] = {s->cx, s->cy}, n[2] = {p.nx, p.ny};
  const char* const nm[2] = {"x", "y"};
  for (int d = 0; d < 2; ++d) {
    if (cxy[d] != 1 && cxy[d] != 2 && cxy[d] != 4 && cxy[d] != 8) {
      err = std::string("snapshot: c") + nm[d] + " = " + std::to_string(cxy[d]) + " is not 1, 2, 4 or 8";
      return EKPNP_ERR_INVALID;
    }
    if (n[d] < 1 || n[d] % cxy[d] != 0) {
      err = std::string("snapshot: c") + nm[d] + " = " + std::to_string(cxy[d]) + " does not divide n" + nm[d] + " = " + std::to_string(n[d]);
      return EKPNP_ERR_INVALID;
    }
  }
  if (s->cz < 1 || p.nz < 2 || (p.nz - 1) % s->cz != 0) {
    err = "snapshot: cz = " + std::to_string(s->cz) + " does not divide nz - 1 = " + std::to_string(p.nz - 1);
    return EKPNP_ERR_INVALID;
  }
  return EKPNP_OK;
}

// output planes k with k*cz in [z0, z0 + nzl)
static void sampled_planes(int z0, int nzl, int cz, int* k0, int* kn) {
  const int first = (z0 + cz - 1) / cz, last = (z0 + nzl - 1) / cz;
  *k0 = first;
  *kn = nzl > 0 && last >= first ? last - first + 1 : 0;
}

int snapshot_write_header(FILE* f, const ekpnp_params& p, const ekpnp_snapshot_spec& s, double time, int k0, int kn) {
  const int X = p.nx / s.cx, Y = p.ny / s.cy;
  std::fprintf(f, "# vtk DataFile Version 3.0\n");
  std::fprintf(f, "ekpnp snapshot time %.17g nx %d ny %d nz %d coarsen %d %d %d z_first %d\n", time, p.nx, p.ny, p.nz, s.cx, s.cy, s.cz, k0);
  std::fprintf(f, "BINARY\nDATASET STRUCTURED_POINTS\nDIMENSIONS %d %d %d\n", X, Y, kn);
  std::fprintf(f, "ORIGIN %.17g %.17g %.17g\n", (s.cx - 1) * p.dx / 2, (s.cy - 1) * p.dy / 2, (double)k0 * s.cz * p.dz);
  std::fprintf(f, "SPACING %.17g %.17g %.17g\n", s.cx * p.dx, s.cy * p.dy, s.cz * p.dz);
  std::fprintf(f, "POINT_DATA %lld\n", (long long)X * Y * kn);
  return std::ferror(f) ? EKPNP_ERR_INVALID : EKPNP_OK;
}

int snapshot_write_field_header(FILE* f, int field_id) {
  std::fprintf(f, "SCALARS %s float 1\nLOOKUP_TABLE default\n", kSnapNames[field_id]);
  return std::ferror(f) ? EKPNP_ERR_INVALID : EKPNP_OK;
}

}  // namespace ekpnp

// the side stream and the events, once per context and only when a snapshot is first asked for
static int need_state(Ctx& c) {
  if (c.snap) return EKPNP_OK;
  SnapState* s = new (std::nothrow) SnapState();
  if (!s) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  c.snap = s;  // (what exists of it is released by snapshot_release, whatever fails below)
  HIPCHK(c, hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
  for (SnapSlot& t : s->slot) {
    HIPCHK(c, hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&t.landed, hipEventDisableTiming));
  }
  return EKPNP_OK;
}

// slot buffers of at least `bytes`; the slot is not pending (its last copy is waited for before the buffers go)
static int need_slot(Ctx& c, SnapSlot& t, size_t bytes) {
  if (t.cap >= bytes) return EKPNP_OK;
  if (t.used) HIPCHK(c, hipEventSynchronize(t.landed));
  if (t.dev) { (void)hipFree(t.dev); c.bytes -= t.cap; }
  if (t.host) (void)hipHostFree(t.host);
  t.dev = nullptr;
  t.host = nullptr;
  t.cap = 0;
  HIPCHK(c, hipMalloc((void**)&t.dev, bytes));
  hipError_t e = hipHostMalloc((void**)&t.host, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipFree(t.dev);
    t.dev = nullptr;
    t.host = nullptr;
    HIPCHK(c, e);
  }
  t.cap = bytes;
  c.bytes += bytes;
  return EKPNP_OK;
}

template <int CX>
static void launch_snapshot_cy(Ctx& c, const SnapFields& a, const SnapGeom& g, int cy, dim3 grid, float* out) {
  const dim3 block(SNAP_LANES, SNAP_ROWS);
  switch (cy) {
    case 1: hipLaunchKernelGGL((k_snapshot<CX, 1>), grid, block, 0, c.stream, a, g, out); break;
    case 2: hipLaunchKernelGGL((k_snapshot<CX, 2>), grid, block, 0, c.stream, a, g, out); break;
    case 4: hipLaunchKernelGGL((k_snapshot<CX, 4>), grid, block, 0, c.stream, a, g, out); break;
    default: hipLaunchKernelGGL((k_snapshot<CX, 8>), grid, block, 0, c.stream, a, g, out); break;
  }
}
static void launch_snapshot(Ctx& c, const SnapFields& a, const SnapGeom& g, int cx, int cy, dim3 grid, float* out) {
  switch (cx) {
    case 1: launch_snapshot_cy<1>(c, a, g, cy, grid, out); break;
    case 2: launch_snapshot_cy<2>(c, a, g, cy, grid, out); break;
    case 4: launch_snapshot_cy<4>(c, a, g, cy, grid, out); break;
    default: launch_snapshot_cy<8>(c, a, g, cy, grid, out); break;
  }
  note_launch(c, "k_snapshot");
}

static int finish_oldest(Ctx& c);

namespace ekpnp {

// enqueue one snapshot of this context's sampled planes (path == null: into memory only); never waits for the compute stream
int snapshot_enqueue(Ctx& c, const ekpnp_snapshot_spec& spec, bool big_endian, const char* path, double time) {
  if (int rc = snapshot_check_spec(c.p, &spec, c.err)) return rc;
  if (int rc = need_state(c)) return rc;
  SnapState& s = *c.snap;
  while (s.q.size() >= 2)
    if (int rc = finish_oldest(c)) return rc;
  SnapPending pd;
  pd.spec = spec;
  pd.mask = spec.fields ? spec.fields : SNAP_ALL;
  pd.nf = popcount(pd.mask);
  sampled_planes(c.z0, c.nzl, spec.cz, &pd.k0, &pd.kn);
  const int X = c.p.nx / spec.cx, Y = c.p.ny / spec.cy;
  pd.bytes = (size_t)pd.nf * (size_t)pd.kn * (size_t)Y * (size_t)X * sizeof(float);
  pd.to_file = path != nullptr;
  if (path) pd.path = path;
  pd.time = time;
  pd.slot = s.next;
  if (pd.kn > 65535) return fail(c, "snapshot: more than 65535 sampled planes in one context");
  if (pd.bytes) {
    if (pd.mask & ((1u << EKPNP_PHI) | (1u << EKPNP_EX) | (1u << EKPNP_EY) | (1u << EKPNP_EZ)))
      if (int rc = ensure_efield(c)) return rc;
    SnapSlot& t = s.slot[pd.slot];
    if (int rc = need_slot(c, t, pd.bytes)) return rc;
    if (t.used) HIPCHK(c, hipStreamWaitEvent(c.stream, t.landed, 0));  // the slot's previous copy has left the staging buffer
    SnapFields a{};
    int n = 0;
    for (int i = 0; i < EKPNP_NFIELDS; ++i)
      if (pd.mask & (1u << i)) {
        a.f[n] = c.fld[i];
        if (((uintptr_t)c.fld[i] & 15u) == 0) a.aligned16 |= 1u << n;
        ++n;
      }
    SnapGeom g{};
    g.nx = c.p.nx;
    g.plane = (long long)c.plane;
    g.X = X;
    g.Y = Y;
    g.cz = spec.cz;
    g.swap = big_endian ? 1 : 0;
    g.zl_first = pd.k0 * spec.cz - c.z0;
    g.xchunks = (X + SNAP_LANES - 1) / SNAP_LANES;
    g.inv = 1.0 / (double)(spec.cx * spec.cy);
    const dim3 grid((unsigned)(pd.nf * g.xchunks), (unsigned)((Y + SNAP_ROWS - 1) / SNAP_ROWS), (unsigned)pd.kn);
    launch_snapshot(c, a, g, spec.cx, spec.cy, grid, t.dev);
    if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
    HIPCHK(c, hipEventRecord(t.done, c.stream));
    HIPCHK(c, hipStreamWaitEvent(s.side, t.done, 0));
    HIPCHK(c, hipMemcpyAsync(t.host, t.dev, pd.bytes, hipMemcpyDeviceToHost, s.side));
    HIPCHK(c, hipEventRecord(t.landed, s.side));
    t.used = true;
  }
  s.next ^= 1;
  s.q.push_back(std::move(pd));
  return EKPNP_OK;
}

int snapshot_pending_count(const Ctx& c) { return c.snap ? (int)c.snap->q.size() : 0; }

// wait for the copy of pending snapshot `newest ? back : front` and hand out where it landed
int snapshot_land(Ctx& c, bool newest, const float** host, int* k0, int* kn, size_t* bytes) {
  if (!c.snap || c.snap->q.empty()) return fail(c, "snapshot: nothing pending");
  const SnapPending& pd = newest ? c.snap->q.back() : c.snap->q.front();
  const SnapSlot& t = c.snap->slot[pd.slot];
  if (pd.bytes) HIPCHK(c, hipEventSynchronize(t.landed));
  *host = pd.bytes ? t.host : nullptr;
  if (k0) *k0 = pd.k0;
  if (kn) *kn = pd.kn;
  if (bytes) *bytes = pd.bytes;
  return EKPNP_OK;
}

void snapshot_pop(Ctx& c, bool newest) {
  if (!c.snap || c.snap->q.empty()) return;
  if (newest) {
    c.snap->next = c.snap->q.back().slot;  // the slot is free again, and the older pending one holds the other
    c.snap->q.pop_back();
  } else {
    c.snap->q.pop_front();
  }
}

// ekpnp_destroy: pending snapshots are discarded once their copies have landed (nothing is written), everything is freed
void snapshot_release(Ctx& c) {
  if (!c.snap) return;
  SnapState* s = c.snap;
  if (s->side) (void)hipStreamSynchronize(s->side);
  for (SnapSlot& t : s->slot) {
    if (t.dev) { (void)hipFree(t.dev); c.bytes -= t.cap; }
    if (t.host) (void)hipHostFree(t.host);
    if (t.done) (void)hipEventDestroy(t.done);
    if (t.landed) (void)hipEventDestroy(t.landed);
  }
  if (s->side) (void)hipStreamDestroy(s->side);
  delete s;
  c.snap = nullptr;
}

}  // namespace ekpnp

// land the oldest pending snapshot, write its file (this context's planes), drop it whatever happened
static int finish_oldest(Ctx& c) {
  const float* h = nullptr;
  int rc = snapshot_land(c, false, &h, nullptr, nullptr, nullptr);
  const SnapPending pd = c.snap->q.front();
  snapshot_pop(c, false);
  if (rc) return rc;
  if (!pd.to_file || pd.kn == 0) return EKPNP_OK;  // a slab that holds no sampled plane writes no file
  FILE* f = std::fopen(pd.path.c_str(), "wb");
  if (!f) { c.err = "snapshot: cannot open " + pd.path; return EKPNP_ERR_INVALID; }
  snapshot_write_header(f, c.p, pd.spec, pd.time, pd.k0, pd.kn);
  const size_t per_field = pd.bytes / (size_t)pd.nf;
  int n = 0;
  for (int i = 0; i < EKPNP_NFIELDS; ++i)
    if (pd.mask & (1u << i)) {
      snapshot_write_field_header(f, i);
      std::fwrite((const char*)h + (size_t)n * per_field, 1, per_field, f);
      ++n;
    }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { c.err = "snapshot: write error on " + pd.path; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

extern "C" int ekpnp_snapshot_extent(const ekpnp_params* p, const ekpnp_snapshot_spec* s, int* X, int* Y, int* Z, size_t* payload_bytes) {
  std::string err;
  if (!p) { set_create_error("snapshot: NULL params"); return EKPNP_ERR_INVALID; }
  if (int rc = snapshot_check_spec(*p, s, err)) { set_create_error(err); return rc; }
  const int x = p->nx / s->cx, y = p->ny / s->cy, z = (p->nz - 1) / s->cz + 1;
  if (X) *X = x;
  if (Y) *Y = y;
  if (Z) *Z = z;
  if (payload_bytes) *payload_bytes = (size_t)popcount(s->fields ? s->fields : SNAP_ALL) * (size_t)x * (size_t)y * (size_t)z * sizeof(float);
  return EKPNP_OK;
}

extern "C" int ekpnp_snapshot_read(ekpnp_ctx* ctx, const ekpnp_snapshot_spec* spec, float* host_out, int* z_first, int* z_count) {
  NEEDCTX(ctx);
  if (!spec || !host_out || !z_first || !z_count) return fail(c, "snapshot: NULL pointer");
  if (int rc = snapshot_enqueue(c, *spec, false, nullptr, 0.0)) return rc;
  const float* h = nullptr;
  size_t bytes = 0;
  int rc = snapshot_land(c, true, &h, z_first, z_count, &bytes);
  if (rc == EKPNP_OK && bytes) std::memcpy(host_out, h, bytes);
  snapshot_pop(c, true);
  return rc;
}

extern "C" int ekpnp_snapshot_begin(ekpnp_ctx* ctx, const ekpnp_snapshot_spec* spec, const char* path, double time) {
  NEEDCTX(ctx);
  if (!spec || !path) return fail(c, "snapshot: NULL pointer");
  return snapshot_enqueue(c, *spec, true, path, time);
}

extern "C" int ekpnp_snapshot_finish(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  int first = EKPNP_OK;
  std::string msg;
  while (snapshot_pending_count(c) > 0) {
    const int rc = finish_oldest(c);
    if (rc && !first) { first = rc; msg = c.err; }
  }
  if (first) c.err = msg;
  return first;
}

extern "C" int ekpnp_snapshot_pending(const ekpnp_ctx* ctx) { return ctx ? snapshot_pending_count(ctx->c) : 0; }
