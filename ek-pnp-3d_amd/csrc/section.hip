// section.hip — vertical sections and space-time lines of the fields: a value summed along ONE horizontal axis over an index range
// lo .. hi, per z plane (include/ekpnp.h: ekpnp_section_sum, ekpnp_section_spec_check, ekpnp_section_extent, ekpnp_section,
// ekpnp_section_save, ekpnp_section_*; no reference counterpart).
//
// THE definition is the host function ekpnp_section_sum: the terms of a line are cut into runs of 64 consecutive indices, a run
// is added in ascending index, the run sums are added in ascending run.  Both kernels make exactly these FP64 additions (the
// object is built with -ffp-contract=off, csrc/Makefile PINNED; a first term is ASSIGNED, never added to a zero, so a cut returns
// the field's own bits), one line per thread or lane, so a number depends on its line alone - not on the grid, the buffer mode,
// the decomposition or what is selected beside it.  Nothing is an atomic, nothing goes through a scratch buffer.
//   k_section_y<PAIR>   across y, keeps x.  256 threads along x (coalesced), grid (ceil(nx / 256), plane slots, arrays).  A thread walks
//                       its column lo .. hi run by run, eight loads in flight, and stores the map entry.
//   k_section_x<PAIR>   across x, keeps y.  One wavefront per workgroup, grid (ceil(ny / ROWS), plane slots, arrays).  Run by run the
//                       wavefront loads a tile of ROWS rows x 64 consecutive x with its lanes along x (a row is 512 B contiguous,
//                       sixteen rows in flight), stores it to LDS with a row pitch of 65 doubles and reads it back transposed: lane r
//                       adds row r's run in ascending x, then adds the run sum to its line.  Pitch 65 doubles = 130 dwords: lane r's
//                       ds_read_b64 of column k starts at bank (2 r + 2 k) mod 64, so the 32 lanes of a half cover the 64 banks once.
//                       Rows beyond ny and columns beyond hi are neither loaded nor added (no padding value enters a sum).
//   PAIR                c and cn together: one pass gives the lines of c, of cn and of q = c - cn (one FP64 subtraction per node
//                       before any addition), each only if selected.  ROWS is 64 for one array and 32 for the pair, so that either
//                       tile set is 33 280 B of LDS (a b64 LDS read is issued a half of 32 lanes at a time: 32 rows cost one issue).
// Only the chosen planes and the indices lo .. hi are read; 8-byte loads only (a wavefront's 64 lanes still read 512 contiguous
// bytes), so an array bound at an odd double, an odd plane of an odd lattice and an odd lo need no second path.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950) and timings: DESIGN.md §9, profiles/section_cost.json.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "ring.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int SEC_NVALUES = EKPNP_NFIELDS + 1;
constexpr int SEC_RUN = 64;       // terms per run: THE definition
constexpr int SEC_PITCH = 65;     // doubles per tile row in LDS (odd: the transposed read is conflict-free)
constexpr int SEC_Y_THREADS = 256;
constexpr int SEC_Y_LOADS = 8;    // loads in flight per thread (across y)
constexpr int SEC_X_LOADS = 16;   // rows in flight per wavefront (across x)

static const char* const kSectionNames[SEC_NVALUES] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T", "q"};

// one array (b == null) or the pair c, cn; o*: the value's position among the selected values, -1: not selected
struct SecJob {
  const double* a;
  const double* b;
  int oa, ob, oq, pad_;
};
struct SecArgs {
  SecJob job[EKPNP_NFIELDS];  // the single arrays, blockIdx.z
  SecJob pair;                // c and cn read together (q selected)
  int zl[EKPNP_MAX_SECTION_PLANES];  // local plane of slot j, -1: another slab's (a row of +0.0)
  int all_planes;             // 1: slot j is local plane j
  int np;                     // plane slots
  int nx, ny;
  long long plane;
  int lo, n;                  // first index and number of terms of a line
  int nkeep;
  double* out;                // [nvalues][np][nkeep]
};

__device__ __forceinline__ void section_store(const SecArgs& s, const SecJob& jb, int slot, int k, bool pair, double a, double b, double q) {
  if (jb.oa >= 0) s.out[((long long)jb.oa * s.np + slot) * s.nkeep + k] = a;
  if (pair) {
    if (jb.ob >= 0) s.out[((long long)jb.ob * s.np + slot) * s.nkeep + k] = b;
    if (jb.oq >= 0) s.out[((long long)jb.oq * s.np + slot) * s.nkeep + k] = q;
  }
}

template <bool PAIR>
__global__ void __launch_bounds__(SEC_Y_THREADS) k_section_y(SecArgs s) {
  const SecJob jb = PAIR ? s.pair : s.job[blockIdx.z];
  const int x = blockIdx.x * SEC_Y_THREADS + threadIdx.x, slot = blockIdx.y;
  if (x >= s.nx) return;
  const int zl = s.all_planes ? slot : s.zl[slot];
  if (zl < 0) { section_store(s, jb, slot, x, PAIR, 0.0, 0.0, 0.0); return; }
  const long long first = (long long)zl * s.plane + (long long)s.lo * s.nx + x;
  const double* __restrict__ a = jb.a + first;
  const double* __restrict__ b = PAIR ? jb.b + first : a;
  double Sa = 0.0, Sb = 0.0, Sq = 0.0;
  for (int i0 = 0; i0 < s.n; i0 += SEC_RUN) {
    const int m = s.n - i0 < SEC_RUN ? s.n - i0 : SEC_RUN;
    double ra = 0.0, rb = 0.0, rq = 0.0;
    for (int k0 = 0; k0 < m; k0 += SEC_Y_LOADS) {
      double va[SEC_Y_LOADS], vb[PAIR ? SEC_Y_LOADS : 1];
#pragma unroll
      for (int k = 0; k < SEC_Y_LOADS; ++k) {
        const bool ok = k0 + k < m;
        const long long off = (long long)(i0 + k0 + k) * s.nx;
        va[k] = ok ? a[off] : 0.0;
        if constexpr (PAIR) vb[k] = ok ? b[off] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < SEC_Y_LOADS; ++k) {
        if (k0 + k >= m) continue;
        const bool head = k == 0 && k0 == 0;  // the run's first term is assigned
        ra = head ? va[k] : ra + va[k];
        if constexpr (PAIR) {
          const double t = va[k] - vb[k];
          rb = head ? vb[k] : rb + vb[k];
          rq = head ? t : rq + t;
        }
      }
    }
    Sa = i0 == 0 ? ra : Sa + ra;
    if constexpr (PAIR) {
      Sb = i0 == 0 ? rb : Sb + rb;
      Sq = i0 == 0 ? rq : Sq + rq;
    }
  }
  section_store(s, jb, slot, x, PAIR, Sa, Sb, Sq);
}

template <bool PAIR>
__global__ void __launch_bounds__(64) k_section_x(SecArgs s) {
  constexpr int ROWS = PAIR ? 32 : 64;
  __shared__ double tile[(PAIR ? 2 : 1) * ROWS * SEC_PITCH];
  double* __restrict__ ta = tile;
  double* __restrict__ tb = PAIR ? tile + ROWS * SEC_PITCH : tile;
  const SecJob jb = PAIR ? s.pair : s.job[blockIdx.z];
  const int lane = threadIdx.x, slot = blockIdx.y;
  const int y0 = blockIdx.x * ROWS;
  const int nrows = s.ny - y0 < ROWS ? s.ny - y0 : ROWS;  // >= 1 by the grid
  const int zl = s.all_planes ? slot : s.zl[slot];
  if (zl < 0) {
    if (lane < nrows) section_store(s, jb, slot, y0 + lane, PAIR, 0.0, 0.0, 0.0);
    return;
  }
  const long long first = (long long)zl * s.plane + (long long)y0 * s.nx + s.lo;
  const double* __restrict__ a = jb.a + first;
  const double* __restrict__ b = PAIR ? jb.b + first : a;
  double Sa = 0.0, Sb = 0.0, Sq = 0.0;
  for (int i0 = 0; i0 < s.n; i0 += SEC_RUN) {
    const int m = s.n - i0 < SEC_RUN ? s.n - i0 : SEC_RUN;
    for (int r0 = 0; r0 < nrows; r0 += SEC_X_LOADS) {
      double va[SEC_X_LOADS], vb[PAIR ? SEC_X_LOADS : 1];
#pragma unroll
      for (int k = 0; k < SEC_X_LOADS; ++k) {
        const bool ok = r0 + k < nrows && lane < m;
        const long long off = (long long)(r0 + k) * s.nx + i0 + lane;
        va[k] = ok ? a[off] : 0.0;
        if constexpr (PAIR) vb[k] = ok ? b[off] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < SEC_X_LOADS; ++k) {  // (r0 + k < ROWS: ROWS is a multiple of SEC_X_LOADS)
        ta[(r0 + k) * SEC_PITCH + lane] = va[k];
        if constexpr (PAIR) tb[(r0 + k) * SEC_PITCH + lane] = vb[k];
      }
    }
    __syncthreads();
    double ra = 0.0, rb = 0.0, rq = 0.0;
    if (lane < nrows) {  // lane r: row r's run in ascending x; entries k >= m and rows >= nrows are never read
      const double* pa = ta + lane * SEC_PITCH;
      const double* pb = tb + lane * SEC_PITCH;
      ra = pa[0];
      if constexpr (PAIR) { rb = pb[0]; rq = ra - rb; }
#pragma unroll 8
      for (int k = 1; k < m; ++k) {
        const double u = pa[k];
        ra = ra + u;
        if constexpr (PAIR) {
          const double v = pb[k];
          rb = rb + v;
          rq = rq + (u - v);
        }
      }
    }
    Sa = i0 == 0 ? ra : Sa + ra;
    if constexpr (PAIR) {
      Sb = i0 == 0 ? rb : Sb + rb;
      Sq = i0 == 0 ? rq : Sq + rq;
    }
    __syncthreads();  // the next run overwrites the tile
  }
  if (lane < nrows) section_store(s, jb, slot, y0 + lane, PAIR, Sa, Sb, Sq);
}

// Host side of a context's sections: made by the first ekpnp_section / ekpnp_section_save / ekpnp_section_arm, never by a context that uses none.
struct SectionState {
  double* out = nullptr;   // the map of the last synchronous call; grows to the largest seen
  size_t out_bytes = 0;
  Ring ring;               // rows of [nvalues][nplanes][nkeep] doubles
  ekpnp_section_spec spec{};
};

static inline uint32_t section_mask(const ekpnp_section_spec& s) { return s.values ? s.values : (1u << SEC_NVALUES) - 1u; }

int section_check_spec(const ekpnp_params& p, const ekpnp_section_spec* s, std::string& err) {
  if (!s) { err = "section: NULL spec"; return EKPNP_ERR_INVALID; }
  if (p.nx < 1 || p.ny < 1 || p.nz < 1) {
    err = "section: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + ", nz = " + std::to_string(p.nz) + " (must be >= 1)";
    return EKPNP_ERR_INVALID;
  }
  if (s->values >> SEC_NVALUES) { err = "section: values = " + std::to_string(s->values) + " selects an id above 11"; return EKPNP_ERR_INVALID; }
  if (s->across != EKPNP_ACROSS_X && s->across != EKPNP_ACROSS_Y) { err = "section: across = " + std::to_string(s->across) + " outside 0 .. 1"; return EKPNP_ERR_INVALID; }
  const int len = s->across == EKPNP_ACROSS_X ? p.nx : p.ny;
  if (s->lo < 0 || s->lo >= len) { err = "section: lo = " + std::to_string(s->lo) + " outside 0 .. " + std::to_string(len - 1); return EKPNP_ERR_INVALID; }
  if (s->hi < 0 || s->hi >= len) { err = "section: hi = " + std::to_string(s->hi) + " outside 0 .. " + std::to_string(len - 1); return EKPNP_ERR_INVALID; }
  if (s->lo > s->hi) { err = "section: lo = " + std::to_string(s->lo) + " above hi = " + std::to_string(s->hi); return EKPNP_ERR_INVALID; }
  if (s->nplanes < 0 || s->nplanes > EKPNP_MAX_SECTION_PLANES) {
    err = "section: nplanes = " + std::to_string(s->nplanes) + " outside 0 .. " + std::to_string(EKPNP_MAX_SECTION_PLANES);
    return EKPNP_ERR_INVALID;
  }
  for (int j = 0; j < s->nplanes; ++j) {
    if (s->z[j] < 0 || s->z[j] >= p.nz) { err = "section: z = " + std::to_string(s->z[j]) + " outside 0 .. " + std::to_string(p.nz - 1); return EKPNP_ERR_INVALID; }
    if (j > 0 && s->z[j] <= s->z[j - 1]) {
      err = "section: z = " + std::to_string(s->z[j]) + " after z = " + std::to_string(s->z[j - 1]) + " (the planes must be strictly ascending)";
      return EKPNP_ERR_INVALID;
    }
  }
  return EKPNP_OK;
}

int section_check_ring(const ekpnp_section_spec& s, int capacity, std::string& err) {
  if (s.nplanes < 1) { err = "section: nplanes = " + std::to_string(s.nplanes) + " (a time series needs 1 .. 16 chosen planes)"; return EKPNP_ERR_INVALID; }
  if (capacity < 1) { err = "section: capacity = " + std::to_string(capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

int section_nvalues(const ekpnp_section_spec& s) { return __builtin_popcount(section_mask(s)); }
int section_nkeep(const ekpnp_params& p, const ekpnp_section_spec& s) { return s.across == EKPNP_ACROSS_X ? p.ny : p.nx; }

const ekpnp_section_spec* section_armed_spec(const Ctx& c) { return c.section && c.section->ring.ever_armed ? &c.section->spec : nullptr; }
bool section_armed(const Ctx& c) { return c.section && c.section->ring.armed; }

void section_release(Ctx& c) {
  if (!c.section) return;
  if (c.section->out) (void)hipFree(c.section->out);
  ring_release(c.section->ring);
  delete c.section;
  c.section = nullptr;
}

static void section_write_head(FILE* f, const ekpnp_params& p, const ekpnp_section_spec& s) {
  std::fprintf(f, "# ekpnp section nx %d ny %d nz %d across %s lo %d hi %d values", p.nx, p.ny, p.nz, s.across == EKPNP_ACROSS_X ? "x" : "y", s.lo, s.hi);
  const uint32_t mask = section_mask(s);
  for (int v = 0; v < SEC_NVALUES; ++v)
    if ((mask >> v) & 1u) std::fprintf(f, " %s", kSectionNames[v]);
  std::fprintf(f, " nkeep %d", section_nkeep(p, s));
}

// the rows "name z v ..." of one map [nvalues][np][nkeep], each behind `lead`
static void section_write_rows(FILE* f, const ekpnp_params& p, const ekpnp_section_spec& s, int np, const int* z, const char* lead, const double* values) {
  const uint32_t mask = section_mask(s);
  const size_t nkeep = (size_t)section_nkeep(p, s);
  int o = 0;
  for (int v = 0; v < SEC_NVALUES; ++v) {
    if (!((mask >> v) & 1u)) continue;
    for (int j = 0; j < np; ++j) {
      const double* row = values + ((size_t)o * np + j) * nkeep;
      std::fprintf(f, "%s%s %d", lead, kSectionNames[v], z[j]);
      for (size_t k = 0; k < nkeep; ++k) std::fprintf(f, " %.17g", row[k]);
      std::fprintf(f, "\n");
    }
    ++o;
  }
}

int section_write_file(const char* path, const ekpnp_params& p, const ekpnp_section_spec& spec, int np, const int* z, double time, const double* values,
                       std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open section file"; return EKPNP_ERR_INVALID; }
  section_write_head(f, p, spec);
  std::fprintf(f, " time %.17g\n", time);
  section_write_rows(f, p, spec, np, z, "", values);
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on section file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

int section_write_ring_file(const char* path, const ekpnp_params& p, const ekpnp_section_spec& spec, int64_t recorded, int64_t dropped, int n,
                            const int64_t* steps, const double* times, const double* values, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open section file"; return EKPNP_ERR_INVALID; }
  section_write_head(f, p, spec);
  std::fprintf(f, " planes");
  for (int j = 0; j < spec.nplanes; ++j) std::fprintf(f, " %d", spec.z[j]);
  std::fprintf(f, " recorded %lld dropped %lld\n", (long long)recorded, (long long)dropped);
  const size_t row = (size_t)section_nvalues(spec) * spec.nplanes * section_nkeep(p, spec);
  char lead[64];
  for (int r = 0; r < n; ++r) {
    std::snprintf(lead, sizeof lead, "%lld %.17g ", (long long)steps[r], times[r]);
    section_write_rows(f, p, spec, spec.nplanes, spec.z, lead, values + (size_t)r * row);
  }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on section file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

}  // namespace ekpnp

static int need_section(Ctx& c) {
  if (c.section) return EKPNP_OK;
  if (c.nzl > 65535) return fail(c, "section: more than 65535 planes in one context");
  c.section = new (std::nothrow) SectionState();
  if (!c.section) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  return EKPNP_OK;
}

// the output buffer at least this large; growing waits for the stream first (the copy of an earlier call may still read it)
static int section_out(Ctx& c, size_t bytes) {
  SectionState& h = *c.section;
  if (bytes <= h.out_bytes) return EKPNP_OK;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  if (h.out) { (void)hipFree(h.out); c.bytes -= h.out_bytes; h.out = nullptr; h.out_bytes = 0; }
  HIPCHK(c, hipMalloc((void**)&h.out, bytes));
  h.out_bytes = bytes;
  c.bytes += bytes;
  return EKPNP_OK;
}

static inline int section_np(const Ctx& c, const ekpnp_section_spec& s) { return s.nplanes ? s.nplanes : c.nzl; }
static inline size_t section_doubles(const Ctx& c, const ekpnp_section_spec& s) {
  return (size_t)section_nvalues(s) * (size_t)section_np(c, s) * (size_t)section_nkeep(c.p, s);
}
static bool section_owns_a_plane(const Ctx& c, const ekpnp_section_spec& s) {
  if (!s.nplanes) return true;
  for (int j = 0; j < s.nplanes; ++j)
    if (s.z[j] >= c.z0 && s.z[j] < c.z0 + c.nzl) return true;
  return false;
}

// enqueue the map [nvalues][np][nkeep] of a checked spec into `out` (device memory, large enough)
static int section_enqueue(Ctx& c, const ekpnp_section_spec& s, double* out) {
  const uint32_t mask = section_mask(s);
  if (mask & ((1u << EKPNP_PHI) | (1u << EKPNP_EX) | (1u << EKPNP_EY) | (1u << EKPNP_EZ))) {
    if (int rc = ensure_efield(c)) return rc;  // the arrays as ekpnp_get_field would return them
  }
  SecArgs a{};
  int pos[SEC_NVALUES], o = 0;
  for (int v = 0; v < SEC_NVALUES; ++v) pos[v] = (mask >> v) & 1u ? o++ : -1;
  const bool pair = pos[EKPNP_SECTION_Q] >= 0;
  int nsingle = 0;
  for (int v = 0; v < EKPNP_NFIELDS; ++v) {
    if (pos[v] < 0 || (pair && (v == EKPNP_C || v == EKPNP_CN))) continue;
    a.job[nsingle++] = SecJob{c.fld[v], nullptr, pos[v], -1, -1, 0};
  }
  a.pair = SecJob{c.fld[EKPNP_C], c.fld[EKPNP_CN], pos[EKPNP_C], pos[EKPNP_CN], pos[EKPNP_SECTION_Q], 0};
  a.all_planes = s.nplanes == 0;
  a.np = section_np(c, s);
  for (int j = 0; j < EKPNP_MAX_SECTION_PLANES; ++j) a.zl[j] = j < s.nplanes && s.z[j] >= c.z0 && s.z[j] < c.z0 + c.nzl ? s.z[j] - c.z0 : -1;
  a.nx = c.p.nx;
  a.ny = c.p.ny;
  a.plane = (long long)c.plane;
  a.lo = s.lo;
  a.n = s.hi - s.lo + 1;
  a.nkeep = section_nkeep(c.p, s);
  a.out = out;
  if (s.across == EKPNP_ACROSS_Y) {
    const unsigned gx = (unsigned)((a.nx + SEC_Y_THREADS - 1) / SEC_Y_THREADS);
    if (nsingle) {
      hipLaunchKernelGGL((k_section_y<false>), dim3(gx, a.np, nsingle), dim3(SEC_Y_THREADS), 0, c.stream, a);
      note_launch(c, "k_section_y");
    }
    if (pair) {
      hipLaunchKernelGGL((k_section_y<true>), dim3(gx, a.np, 1), dim3(SEC_Y_THREADS), 0, c.stream, a);
      note_launch(c, "k_section_y");
    }
  } else {
    if (nsingle) {
      hipLaunchKernelGGL((k_section_x<false>), dim3((a.ny + 63) / 64, a.np, nsingle), dim3(64), 0, c.stream, a);
      note_launch(c, "k_section_x");
    }
    if (pair) {
      hipLaunchKernelGGL((k_section_x<true>), dim3((a.ny + 31) / 32, a.np, 1), dim3(64), 0, c.stream, a);
      note_launch(c, "k_section_x");
    }
  }
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" double ekpnp_section_sum(const double* v, ptrdiff_t stride, int n) {
  double S = 0.0;
  for (int i0 = 0; i0 < n; i0 += SEC_RUN) {
    const int end = i0 + SEC_RUN < n ? i0 + SEC_RUN : n;
    double r = v[(ptrdiff_t)i0 * stride];
    for (int i = i0 + 1; i < end; ++i) r = r + v[(ptrdiff_t)i * stride];
    S = i0 == 0 ? r : S + r;
  }
  return S;
}

extern "C" int ekpnp_section_spec_check(const ekpnp_params* p, const ekpnp_section_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "section: NULL parameters";
  else rc = section_check_spec(*p, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_section_extent(const ekpnp_params* p, const ekpnp_section_spec* spec, int* nvalues, int* nkeep) {
  if (int rc = ekpnp_section_spec_check(p, spec)) return rc;
  if (!nvalues || !nkeep) { set_create_error("section: NULL pointer"); return EKPNP_ERR_INVALID; }
  *nvalues = section_nvalues(*spec);
  *nkeep = section_nkeep(*p, *spec);
  return EKPNP_OK;
}

extern "C" int ekpnp_section(ekpnp_ctx* ctx, const ekpnp_section_spec* spec, double* host_out) {
  NEEDCTX(ctx);
  if (!host_out) return fail(c, "NULL pointer");
  if (int rc = section_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = need_section(c)) return rc;
  const size_t n = section_doubles(c, *spec);
  if (!section_owns_a_plane(c, *spec)) {  // no chosen plane here: rows of +0.0, no kernel reads a field
    for (size_t i = 0; i < n; ++i) host_out[i] = 0.0;
    return EKPNP_OK;
  }
  if (int rc = section_out(c, n * sizeof(double))) return rc;
  if (int rc = section_enqueue(c, *spec, c.section->out)) return rc;
  HIPCHK(c, hipMemcpyAsync(host_out, c.section->out, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_section_save(ekpnp_ctx* ctx, const ekpnp_section_spec* spec, const char* path, double time) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  if (int rc = section_check_spec(c.p, spec, c.err)) return rc;
  std::vector<double> v(section_doubles(c, *spec));
  if (int rc = ekpnp_section(ctx, spec, v.data())) return rc;
  const int np = section_np(c, *spec);
  std::vector<int> z((size_t)np);
  for (int j = 0; j < np; ++j) z[(size_t)j] = spec->nplanes ? spec->z[j] : c.z0 + j;
  return section_write_file(path, c.p, *spec, np, z.data(), time, v.data(), c.err);
}

extern "C" int ekpnp_section_arm(ekpnp_ctx* ctx, const ekpnp_section_spec* spec, int capacity) {
  NEEDCTX(ctx);
  if (int rc = section_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = section_check_ring(*spec, capacity, c.err)) return rc;
  if (int rc = need_section(c)) return rc;
  SectionState& h = *c.section;
  h.spec = *spec;
  return ring_arm(c, h.ring, capacity, section_doubles(c, *spec) * sizeof(double));
}

extern "C" int ekpnp_section_disarm(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (c.section) c.section->ring.armed = false;  // the ring and its rows stay readable until the next arm
  return EKPNP_OK;
}

extern "C" int ekpnp_section_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDCTX(ctx);
  if (!c.section || !c.section->ring.armed) return fail(c, "ekpnp_section_record: no section armed");
  SectionState& h = *c.section;
  const size_t row = section_doubles(c, h.spec);
  double* out = (double*)ring_next_row(h.ring);
  if (!section_owns_a_plane(c, h.spec)) {  // no chosen plane here: rows of +0.0, no kernel reads a field
    HIPCHK(c, hipMemsetAsync(out, 0, row * sizeof(double), c.stream));
  } else if (int rc = section_enqueue(c, h.spec, out)) {
    return rc;
  }
  ring_note_row(h.ring, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_section_count(const ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  if (!ctx) return EKPNP_ERR_INVALID;
  ring_count(ctx->c.section ? &ctx->c.section->ring : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_section_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, double* values) {
  NEEDCTX(ctx);
  return ring_read(c, c.section ? &c.section->ring : nullptr, "ekpnp_section_read", first, count, steps, times, values);
}

extern "C" int ekpnp_section_ring_save(ekpnp_ctx* ctx, const char* path) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  const ekpnp_section_spec* spec = section_armed_spec(c);
  if (!spec) return fail(c, "ekpnp_section_ring_save: no section was armed");
  int64_t rec = 0, dropped = 0;
  (void)ekpnp_section_count(ctx, &rec, &dropped);
  const int n = (int)(rec - dropped);
  std::vector<int64_t> steps((size_t)n);
  std::vector<double> times((size_t)n), values((size_t)n * section_doubles(c, *spec));
  if (int rc = ekpnp_section_read(ctx, 0, n, steps.data(), times.data(), values.data())) return rc;
  return section_write_ring_file(path, c.p, *spec, rec, dropped, n, steps.data(), times.data(), values.data(), c.err);
}
