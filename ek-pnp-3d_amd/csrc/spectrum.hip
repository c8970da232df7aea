// spectrum.hip — x-y power spectra of a field per z plane: shell spectrum E(k), dominant mode, and their time series
// (include/ekpnp.h: ekpnp_spectrum_*; no reference counterpart).
//
// modes.hip projects onto at most 16 modes the caller names in advance; which wavelength an instability SELECTS needs the whole
// spectrum.  The transform is a hipFFT D2Z plan of the plane's extents, of batch B, on buffers of this file's own: a field array is
// never handed to hipFFT (nothing can be overwritten, nothing past the end of an array is read), and the solve's buffers and plans
// are not touched.  Per batch of at most B planes:
//   k_spec_gather   grid (ceil(nx*ny / 256), B): plane slot b of the real staging buffer [B][ny][nx] = the plane the slot names, or
//                   zeros for an unused slot (a short last batch runs the same plan)
//   hipfftExecD2Z   staging -> the complex buffer [B][ny][nxh], on the context's stream
//   k_spec_shells   grid (nshell, slots in use), 256 threads: E(s) = sum of P over the shell's list of modes (CSR table built on
//                   the host from nx, ny, Lx, Ly: ascending linear index n*nxh + m within a shell).  Thread t adds entries t,
//                   t + 256, ... in ascending order, then the wave tree of reduce.h, then the four waves in ascending order
//                   through LDS
//   k_spec_peak     grid (slots in use), 256 threads: argmax of P over all modes but (0, 0) whose P is positive (neither NaN nor
//                   zero); among equals the smallest linear index wins - a total order, so the tree's shape does not matter
// P = w*(re*re + im*im) formed as e = re*re; e = e + im*im; P = w*e (spec_power below, ONE function for the device and for the
// host side of ekpnp_spectrum_plane); the object is built with -ffp-contract=off (csrc/Makefile, PINNED).  No atomics: the order
// of the additions depends on the table alone, that is on nx, ny, Lx, Ly - not on z0, nzl, the buffer mode, the slot or the device.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "reduce.h"
#include "ring.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int SPEC_THREADS = 256;
constexpr int MAXP = EKPNP_MAX_SPECTRUM_PLANES;
constexpr size_t SPEC_BATCH_BYTES = (size_t)64 << 20;  // about this much spectrum per batch

static const char* const kSpecFieldNames[EKPNP_NFIELDS] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"};

__host__ __device__ inline double spec_weight(int m, int nx) { return (m == 0 || ((nx & 1) == 0 && m == nx / 2)) ? 1.0 : 2.0; }
__host__ __device__ inline double spec_power(double re, double im, double w) {
  double e = re * re;
  const double ii = im * im;
  e = e + ii;
  return w * e;
}

// which plane goes into which slot of the batch, and which row of the result the slot's shells and peak go to
struct SpecSlots {
  int zl[MAXP];   // local plane, < 0: the slot is unused (zeroed, its output ignored)
  int row[MAXP];
};

__global__ void __launch_bounds__(SPEC_THREADS) k_spec_gather(const double* __restrict__ fld, long long plane, SpecSlots s, double* __restrict__ stage) {
  const long long i = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
  if (i >= plane) return;
  const int b = blockIdx.y, zl = s.zl[b];
  stage[(long long)b * plane + i] = zl >= 0 ? fld[(long long)zl * plane + i] : 0.0;
}

// shells[row * nshell + s] of slot blockIdx.y
__global__ void __launch_bounds__(SPEC_THREADS) k_spec_shells(const double2* __restrict__ spec, long long nspec, const int* __restrict__ start,
                                                               const int* __restrict__ modes, int nx, int nxh, int nshell, SpecSlots s,
                                                               double* __restrict__ shells) {
  __shared__ double lds[SPEC_THREADS / 64];
  const int sh = blockIdx.x, b = blockIdx.y;
  const double2* __restrict__ F = spec + (long long)b * nspec;
  const int i0 = start[sh], i1 = start[sh + 1];
  double acc = 0.0;
  for (int i = i0 + (int)threadIdx.x; i < i1; i += SPEC_THREADS) {
    const int idx = modes[i];
    const double2 f = F[idx];
    acc = acc + spec_power(f.x, f.y, spec_weight(idx % nxh, nx));
  }
  const double r = wave_sum(acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    double E = lds[0];
#pragma unroll
    for (int w = 1; w < SPEC_THREADS / 64; ++w) E = E + lds[w];
    shells[(long long)s.row[b] * nshell + sh] = E;
  }
}

// a candidate of the argmax: idx < 0 is "none".  Larger P wins, among equals the smaller index: a total order
__device__ __forceinline__ void spec_better(double& P, int& idx, double P2, int idx2) {
  if (idx2 < 0) return;
  if (idx < 0 || P2 > P || (P2 == P && idx2 < idx)) { P = P2; idx = idx2; }
}

// peaks[row * 3 + {0: m, 1: n signed, 2: P}] of slot blockIdx.x
__global__ void __launch_bounds__(SPEC_THREADS) k_spec_peak(const double2* __restrict__ spec, long long nspec, int nx, int ny, int nxh, SpecSlots s,
                                                             double* __restrict__ peaks) {
  __shared__ double ldsP[SPEC_THREADS / 64];
  __shared__ int ldsI[SPEC_THREADS / 64];
  const int b = blockIdx.x;
  const double2* __restrict__ F = spec + (long long)b * nspec;
  double P = 0.0;
  int idx = -1;
  for (long long i = threadIdx.x; i < nspec; i += SPEC_THREADS) {
    if (i == 0) continue;  // the plane mean is no candidate
    const double2 f = F[i];
    const double q = spec_power(f.x, f.y, spec_weight((int)(i % nxh), nx));
    if (q > 0.0) spec_better(P, idx, q, (int)i);  // (false for a NaN too)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double P2 = __shfl_down(P, off, 64);
    const int idx2 = __shfl_down(idx, off, 64);
    spec_better(P, idx, P2, idx2);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { ldsP[wave] = P; ldsI[wave] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    P = ldsP[0];
    idx = ldsI[0];
#pragma unroll
    for (int w = 1; w < SPEC_THREADS / 64; ++w) spec_better(P, idx, ldsP[w], ldsI[w]);
    double* out = peaks + (long long)s.row[b] * 3;
    if (idx < 0) {
      out[0] = 0.0; out[1] = 0.0; out[2] = 0.0;
    } else {
      const int m = idx % nxh, n = idx / nxh;
      out[0] = (double)m;
      out[1] = (double)(n > ny / 2 ? n - ny : n);
      out[2] = P;
    }
  }
}

// The shell table of a plane geometry (include/ekpnp.h has the definition): shell_of [ny][nxh] and the CSR list of each shell's modes
struct ShellTable {
  int nshell = 0;
  double L = 0.0;
  std::vector<int32_t> shell_of;  // [ny][nxh]
  std::vector<int32_t> start;     // [nshell + 1]
  std::vector<int32_t> modes;     // [ny * nxh]: linear indices, ascending within a shell
};

static int shell_table(const ekpnp_params& p, ShellTable& t, std::string& err) {
  if (p.nx < 1 || p.ny < 1) { err = "spectrum: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (!(p.Lx > 0.0 && p.Ly > 0.0)) { err = "spectrum: Lx = " + std::to_string(p.Lx) + ", Ly = " + std::to_string(p.Ly) + " (must be positive)"; return EKPNP_ERR_INVALID; }
  const int nx = p.nx, ny = p.ny, nxh = nx / 2 + 1;
  if ((long long)ny * nxh > (long long)INT_MAX / 2) { err = "spectrum: " + std::to_string((long long)ny * nxh) + " modes in a plane (too many)"; return EKPNP_ERR_INVALID; }
  const double L = p.Lx > p.Ly ? p.Lx : p.Ly, rx = L / p.Lx, ry = L / p.Ly;
  t.L = L;
  t.shell_of.resize((size_t)ny * nxh);
  int smax = 0;
  for (int n = 0; n < ny; ++n) {
    const int ns = n > ny / 2 ? n - ny : n;
    for (int m = 0; m < nxh; ++m) {
      const double a = (double)m * rx, b = (double)ns * ry;
      const double aa = a * a, bb = b * b;
      const double k2 = aa + bb;
      const double r = std::sqrt(k2) + 0.5;
      if (!(r < 1.0e9)) { err = "spectrum: shell index " + std::to_string(r) + " (Lx and Ly differ too much)"; return EKPNP_ERR_INVALID; }
      const int s = (int)std::floor(r);
      t.shell_of[(size_t)n * nxh + m] = s;
      if (s > smax) smax = s;
    }
  }
  t.nshell = 1 + smax;
  t.start.assign((size_t)t.nshell + 1, 0);
  for (int32_t s : t.shell_of) ++t.start[(size_t)s + 1];
  for (int s = 0; s < t.nshell; ++s) t.start[(size_t)s + 1] += t.start[(size_t)s];
  t.modes.resize(t.shell_of.size());
  std::vector<int32_t> fill(t.start.begin(), t.start.end() - 1);
  for (size_t i = 0; i < t.shell_of.size(); ++i) t.modes[(size_t)fill[(size_t)t.shell_of[i]]++] = (int32_t)i;  // ascending i within a shell
  return EKPNP_OK;
}

int spectrum_check_spec(const ekpnp_params& p, const ekpnp_spectrum_spec* s, std::string& err) {
  if (!s) { err = "spectrum: NULL spec"; return EKPNP_ERR_INVALID; }
  if (p.nx < 1 || p.ny < 1 || p.nz < 1) {
    err = "spectrum: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + ", nz = " + std::to_string(p.nz) + " (must be >= 1)";
    return EKPNP_ERR_INVALID;
  }
  if (s->field_id < 0 || s->field_id >= EKPNP_NFIELDS) { err = "spectrum: field_id = " + std::to_string(s->field_id) + " outside 0 .. 10"; return EKPNP_ERR_INVALID; }
  if (s->nplanes < 0 || s->nplanes > MAXP) { err = "spectrum: nplanes = " + std::to_string(s->nplanes) + " outside 0 .. " + std::to_string(MAXP); return EKPNP_ERR_INVALID; }
  for (int j = 0; j < s->nplanes; ++j) {
    if (s->z[j] < 0 || s->z[j] >= p.nz) {
      err = "spectrum: z[" + std::to_string(j) + "] = " + std::to_string(s->z[j]) + " outside 0 .. " + std::to_string(p.nz - 1);
      return EKPNP_ERR_INVALID;
    }
    if (j > 0 && s->z[j] <= s->z[j - 1]) {
      err = "spectrum: z[" + std::to_string(j) + "] = " + std::to_string(s->z[j]) + " does not come after z[" + std::to_string(j - 1) + "] = " + std::to_string(s->z[j - 1]) +
            " (strictly ascending)";
      return EKPNP_ERR_INVALID;
    }
  }
  return EKPNP_OK;
}

// Host side of a context's spectra: made by the first ekpnp_spectrum_plane / ekpnp_spectrum / ekpnp_spectrum_arm, never by a context that uses none.
struct SpecState {
  int B = 1;                     // planes per batch of the plan
  int nshell = 0;
  double L = 0.0;
  size_t nspec = 0;              // ny * nxh
  void* buf = nullptr;           // one allocation: [spectrum | staging | result of a synchronous call | shell table]
  size_t buf_bytes = 0;
  double2* spec = nullptr;       // [B][ny][nxh]
  double* stage = nullptr;       // [B][ny][nx]
  double* res = nullptr;         // [rows][nshell] then [rows][3], rows <= res_rows
  int res_rows = 0;
  int* start = nullptr;          // [nshell + 1]
  int* modes = nullptr;          // [ny * nxh]
  hipfftHandle plan = 0;
  bool have_plan = false;
  size_t plan_bytes = 0;         // the plan's work area
  Ring ring;                     // rows of [nplanes][nshell] then [nplanes][3] doubles
  ekpnp_spectrum_spec spec_armed{};
  ShellTable table;              // (kept while its upload may be in flight)
};

static inline size_t spec_row_doubles(const SpecState& m, int rows) { return (size_t)rows * ((size_t)m.nshell + 3); }

const ekpnp_spectrum_spec* spectrum_armed_spec(const Ctx& c) { return c.spectrum && c.spectrum->ring.ever_armed ? &c.spectrum->spec_armed : nullptr; }

bool spectrum_armed(const Ctx& c) { return c.spectrum && c.spectrum->ring.armed; }

int spectrum_shell_count(const ekpnp_params& p, int* nshell, double* L, std::string& err) {
  ShellTable t;
  if (int rc = shell_table(p, t, err)) return rc;
  if (nshell) *nshell = t.nshell;
  if (L) *L = t.L;
  return EKPNP_OK;
}

void spectrum_release(Ctx& c) {
  if (!c.spectrum) return;
  if (c.spectrum->have_plan) hipfftDestroy(c.spectrum->plan);
  if (c.spectrum->buf) (void)hipFree(c.spectrum->buf);
  ring_release(c.spectrum->ring);
  delete c.spectrum;
  c.spectrum = nullptr;
}

// ekpnp_set_stream: the plan follows the context's stream, as the solve's plans do
int spectrum_set_stream(Ctx& c) {
  if (!c.spectrum || !c.spectrum->have_plan) return EKPNP_OK;
  const hipfftResult r = hipfftSetStream(c.spectrum->plan, c.stream);
  if (r != HIPFFT_SUCCESS) { c.err = "hipfftSetStream (spectrum) failed: " + std::to_string((int)r); return EKPNP_ERR_FFT; }
  return EKPNP_OK;
}

int spectrum_write_file(const char* path, const ekpnp_params& p, const ekpnp_spectrum_spec& spec, int nshell, double L, int64_t recorded, int64_t dropped,
                        int n, const int64_t* steps, const double* times, const double* shells, const double* peaks, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = "cannot open spectrum file"; return EKPNP_ERR_INVALID; }
  std::fprintf(f, "# ekpnp spectrum nx %d ny %d nz %d field %s planes", p.nx, p.ny, p.nz, kSpecFieldNames[spec.field_id]);
  for (int j = 0; j < spec.nplanes; ++j) std::fprintf(f, " %d", spec.z[j]);
  std::fprintf(f, " nshell %d L %.17g recorded %lld dropped %lld\n", nshell, L, (long long)recorded, (long long)dropped);
  std::fprintf(f, "# step time z peak_m peak_n peak_P");
  for (int s = 0; s < nshell; ++s) std::fprintf(f, " E_%d", s);
  std::fprintf(f, "\n");
  for (int r = 0; r < n; ++r)
    for (int j = 0; j < spec.nplanes; ++j) {
      const double* pk = peaks + ((size_t)r * spec.nplanes + j) * 3;
      const double* sh = shells + ((size_t)r * spec.nplanes + j) * nshell;
      std::fprintf(f, "%lld %.17g %lld %lld %lld %.17g", (long long)steps[r], times[r], (long long)spec.z[j], (long long)pk[0], (long long)pk[1], pk[2]);
      for (int s = 0; s < nshell; ++s) std::fprintf(f, " %.17g", sh[s]);
      std::fprintf(f, "\n");
    }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) { err = "write error on spectrum file"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

}  // namespace ekpnp

static inline size_t even(size_t n) { return (n + 1) & ~(size_t)1; }

// the host state, the plan, its two buffers, the result rows and the shell table, once
static int need_spectrum(Ctx& c) {
  if (c.spectrum) return EKPNP_OK;
  if (c.nzl > 65535) return fail(c, "spectrum: more than 65535 planes in one context");
  SpecState* m = new (std::nothrow) SpecState();
  if (!m) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  if (int rc = shell_table(c.p, m->table, c.err)) { delete m; return rc; }
  const int nx = c.p.nx, ny = c.p.ny, nxh = nx / 2 + 1;
  m->nshell = m->table.nshell;
  m->L = m->table.L;
  m->nspec = (size_t)ny * nxh;
  const size_t per_plane = m->nspec * sizeof(double2);
  m->B = (int)(SPEC_BATCH_BYTES / per_plane < 1 ? 1 : SPEC_BATCH_BYTES / per_plane > (size_t)MAXP ? (size_t)MAXP : SPEC_BATCH_BYTES / per_plane);
  m->res_rows = c.nzl > MAXP ? c.nzl : MAXP;
  const size_t nspec_d = 2 * (size_t)m->B * m->nspec, nstage = even((size_t)m->B * c.plane), nres = even(spec_row_doubles(*m, m->res_rows));
  const size_t ntab = (size_t)m->nshell + 1 + m->nspec;
  m->buf_bytes = (nspec_d + nstage + nres) * sizeof(double) + ntab * sizeof(int);
  hipError_t e = hipMalloc(&m->buf, m->buf_bytes);
  if (e != hipSuccess) {
    delete m;
    HIPCHK(c, e);
  }
  m->spec = (double2*)m->buf;
  m->stage = (double*)m->buf + nspec_d;
  m->res = m->stage + nstage;
  m->start = (int*)(m->res + nres);
  m->modes = m->start + m->nshell + 1;
  int n[2] = {ny, nx}, rembed[2] = {ny, nx}, cembed[2] = {ny, nxh};
  const hipfftResult r = hipfftPlanMany(&m->plan, 2, n, rembed, 1, ny * nx, cembed, 1, ny * nxh, HIPFFT_D2Z, m->B);
  if (r != HIPFFT_SUCCESS) {
    (void)hipFree(m->buf);
    delete m;
    c.err = "hipfftPlanMany (spectrum, D2Z) failed: " + std::to_string((int)r);
    return EKPNP_ERR_FFT;
  }
  m->have_plan = true;
  hipfftSetStream(m->plan, c.stream);
  size_t ws = 0;
  if (hipfftGetSize(m->plan, &ws) == HIPFFT_SUCCESS) m->plan_bytes = ws;
  e = hipMemcpyAsync(m->start, m->table.start.data(), ((size_t)m->nshell + 1) * sizeof(int), hipMemcpyHostToDevice, c.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->modes, m->table.modes.data(), m->nspec * sizeof(int), hipMemcpyHostToDevice, c.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e != hipSuccess) {
    hipfftDestroy(m->plan);
    (void)hipFree(m->buf);
    delete m;
    HIPCHK(c, e);
  }
  c.bytes += m->buf_bytes + m->plan_bytes;
  c.spectrum = m;
  return EKPNP_OK;
}

// one batch: the planes of `slots` (nb of them in use, in slots 0 .. nb - 1) gathered and transformed into SpecState::spec
static int spectrum_transform(Ctx& c, int field_id, const SpecSlots& slots) {
  SpecState& m = *c.spectrum;
  const dim3 grid((unsigned)((c.plane + SPEC_THREADS - 1) / SPEC_THREADS), (unsigned)m.B);
  hipLaunchKernelGGL(k_spec_gather, grid, dim3(SPEC_THREADS), 0, c.stream, (const double*)c.fld[field_id], (long long)c.plane, slots, m.stage);
  note_launch(c, "k_spec_gather");
  const hipfftResult r = hipfftExecD2Z(m.plan, m.stage, (hipfftDoubleComplex*)m.spec);
  if (r != HIPFFT_SUCCESS) { c.err = "hipfftExecD2Z (spectrum) failed: " + std::to_string((int)r); return EKPNP_ERR_FFT; }
  return EKPNP_OK;
}

// enqueue shells and peaks of the current field: plane zl[k] of this context into row rows[k] (k < n) of out, which is
// [nrows][nshell] then [nrows][3]; rows nobody names are +0.0 and (0, 0, 0.0)
static int spectrum_enqueue(Ctx& c, int field_id, const int* zl, const int* rows, int n, int nrows, double* out) {
  SpecState& m = *c.spectrum;
  if (field_id == EKPNP_PHI || field_id == EKPNP_EX || field_id == EKPNP_EY || field_id == EKPNP_EZ) {
    if (int rc = ensure_efield(c)) return rc;  // the arrays as ekpnp_get_field would return them
  }
  if (n < nrows) HIPCHK(c, hipMemsetAsync(out, 0, spec_row_doubles(m, nrows) * sizeof(double), c.stream));
  double* shells = out;
  double* peaks = out + (size_t)nrows * m.nshell;
  for (int k0 = 0; k0 < n; k0 += m.B) {
    const int nb = n - k0 < m.B ? n - k0 : m.B;
    SpecSlots slots;
    for (int b = 0; b < MAXP; ++b) {
      slots.zl[b] = b < nb ? zl[k0 + b] : -1;
      slots.row[b] = b < nb ? rows[k0 + b] : 0;
    }
    if (int rc = spectrum_transform(c, field_id, slots)) return rc;
    hipLaunchKernelGGL(k_spec_shells, dim3((unsigned)m.nshell, (unsigned)nb), dim3(SPEC_THREADS), 0, c.stream, (const double2*)m.spec, (long long)m.nspec,
                       (const int*)m.start, (const int*)m.modes, c.p.nx, c.p.nx / 2 + 1, m.nshell, slots, shells);
    note_launch(c, "k_spec_shells");
    hipLaunchKernelGGL(k_spec_peak, dim3((unsigned)nb), dim3(SPEC_THREADS), 0, c.stream, (const double2*)m.spec, (long long)m.nspec, c.p.nx, c.p.ny,
                       c.p.nx / 2 + 1, slots, peaks);
    note_launch(c, "k_spec_peak");
  }
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

// the planes of `spec` this context holds: local plane and result row of each; returns how many, nrows = rows of the result
static int spectrum_held(const Ctx& c, const ekpnp_spectrum_spec& spec, std::vector<int>& zl, std::vector<int>& rows, int* nrows) {
  zl.clear();
  rows.clear();
  if (spec.nplanes == 0) {
    for (int z = 0; z < c.nzl; ++z) { zl.push_back(z); rows.push_back(z); }
    *nrows = c.nzl;
  } else {
    for (int j = 0; j < spec.nplanes; ++j)
      if (spec.z[j] >= c.z0 && spec.z[j] < c.z0 + c.nzl) { zl.push_back(spec.z[j] - c.z0); rows.push_back(j); }
    *nrows = spec.nplanes;
  }
  return (int)zl.size();
}

extern "C" int ekpnp_spectrum_spec_check(const ekpnp_params* p, const ekpnp_spectrum_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "spectrum: NULL parameters";
  else rc = spectrum_check_spec(*p, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_spectrum_shell_count(const ekpnp_params* p, int* nshell) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p || !nshell) err = "spectrum: NULL pointer";
  else rc = spectrum_shell_count(*p, nshell, nullptr, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_spectrum_shells(const ekpnp_params* p, int32_t* shell_of, int32_t* count) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  ShellTable t;
  if (!p || !shell_of) err = "spectrum: NULL pointer";
  else rc = shell_table(*p, t, err);
  if (rc) { set_create_error(err); return rc; }
  std::memcpy(shell_of, t.shell_of.data(), t.shell_of.size() * sizeof(int32_t));
  if (count)
    for (int s = 0; s < t.nshell; ++s) count[s] = t.start[(size_t)s + 1] - t.start[(size_t)s];
  return EKPNP_OK;
}

extern "C" int ekpnp_spectrum_plane(ekpnp_ctx* ctx, int field_id, int z_global, double* power) {
  NEEDCTX(ctx);
  if (!power) return fail(c, "NULL pointer");
  if (field_id < 0 || field_id >= EKPNP_NFIELDS) { c.err = "spectrum: field_id = " + std::to_string(field_id) + " outside 0 .. 10"; return EKPNP_ERR_INVALID; }
  if (z_global < 0 || z_global >= c.p.nz) { c.err = "spectrum: z = " + std::to_string(z_global) + " outside 0 .. " + std::to_string(c.p.nz - 1); return EKPNP_ERR_INVALID; }
  if (z_global < c.z0 || z_global >= c.z0 + c.nzl) {
    c.err = "spectrum: plane z = " + std::to_string(z_global) + " is not held by this context (planes " + std::to_string(c.z0) + " .. " + std::to_string(c.z0 + c.nzl - 1) + ")";
    return EKPNP_ERR_INVALID;
  }
  if (int rc = need_spectrum(c)) return rc;
  SpecState& m = *c.spectrum;
  if (field_id == EKPNP_PHI || field_id == EKPNP_EX || field_id == EKPNP_EY || field_id == EKPNP_EZ) {
    if (int rc = ensure_efield(c)) return rc;
  }
  SpecSlots slots;
  for (int b = 0; b < MAXP; ++b) { slots.zl[b] = b == 0 ? z_global - c.z0 : -1; slots.row[b] = 0; }
  std::vector<double2> F(m.nspec);
  int rc = spectrum_transform(c, field_id, slots);
  if (rc == EKPNP_OK && take_launch_error(c) != hipSuccess) rc = EKPNP_ERR_HIP;
  if (rc == EKPNP_OK) {
    const hipError_t e = hipMemcpyAsync(F.data(), m.spec, m.nspec * sizeof(double2), hipMemcpyDeviceToHost, c.stream);
    if (e != hipSuccess) { c.err = std::string("hipMemcpyAsync: ") + hipGetErrorString(e); rc = EKPNP_ERR_HIP; }
  }
  HIPCHK(c, hipStreamSynchronize(c.stream));  // (also before F goes away)
  if (rc) return rc;
  const int nx = c.p.nx, nxh = nx / 2 + 1;
  for (size_t i = 0; i < m.nspec; ++i) power[i] = spec_power(F[i].x, F[i].y, spec_weight((int)(i % (size_t)nxh), nx));  // the device's expression, rounded alike
  return EKPNP_OK;
}

extern "C" int ekpnp_spectrum(ekpnp_ctx* ctx, const ekpnp_spectrum_spec* spec, double* shells, double* peaks) {
  NEEDCTX(ctx);
  if (!shells) return fail(c, "NULL pointer");
  if (int rc = spectrum_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = need_spectrum(c)) return rc;
  SpecState& m = *c.spectrum;
  std::vector<int> zl, rows;
  int nrows = 0;
  const int n = spectrum_held(c, *spec, zl, rows, &nrows);
  int rc = spectrum_enqueue(c, spec->field_id, zl.data(), rows.data(), n, nrows, m.res);
  if (rc == EKPNP_OK) {
    hipError_t e = hipMemcpyAsync(shells, m.res, (size_t)nrows * m.nshell * sizeof(double), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess && peaks) e = hipMemcpyAsync(peaks, m.res + (size_t)nrows * m.nshell, (size_t)nrows * 3 * sizeof(double), hipMemcpyDeviceToHost, c.stream);
    if (e != hipSuccess) { c.err = std::string("hipMemcpyAsync: ") + hipGetErrorString(e); rc = EKPNP_ERR_HIP; }
  }
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return rc;
}

extern "C" int ekpnp_spectrum_arm(ekpnp_ctx* ctx, const ekpnp_spectrum_spec* spec, int capacity) {
  NEEDCTX(ctx);
  if (int rc = spectrum_check_spec(c.p, spec, c.err)) return rc;
  if (spec->nplanes < 1) { c.err = "spectrum: nplanes = " + std::to_string(spec->nplanes) + " (a time series needs 1 .. " + std::to_string(MAXP) + " chosen planes)"; return EKPNP_ERR_INVALID; }
  if (capacity < 1) { c.err = "spectrum: capacity = " + std::to_string(capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (int rc = need_spectrum(c)) return rc;
  SpecState& m = *c.spectrum;
  m.spec_armed = *spec;
  return ring_arm(c, m.ring, capacity, spec_row_doubles(m, spec->nplanes) * sizeof(double));
}

extern "C" int ekpnp_spectrum_disarm(ekpnp_ctx* ctx) {
  NEEDCTX(ctx);
  if (c.spectrum) c.spectrum->ring.armed = false;  // the ring and its rows stay readable until the next arm
  return EKPNP_OK;
}

extern "C" int ekpnp_spectrum_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDCTX(ctx);
  if (!c.spectrum || !c.spectrum->ring.armed) return fail(c, "ekpnp_spectrum_record: no spectrum tracking armed");
  SpecState& m = *c.spectrum;
  std::vector<int> zl, rows;
  int nrows = 0;
  const int n = spectrum_held(c, m.spec_armed, zl, rows, &nrows);
  if (int rc = spectrum_enqueue(c, m.spec_armed.field_id, zl.data(), rows.data(), n, nrows, (double*)ring_next_row(m.ring))) return rc;
  ring_note_row(m.ring, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_spectrum_count(const ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  if (!ctx) return EKPNP_ERR_INVALID;
  ring_count(ctx->c.spectrum ? &ctx->c.spectrum->ring : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_spectrum_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, double* shells, double* peaks) {
  NEEDCTX(ctx);
  const SpecState* m = c.spectrum;
  const int np = m ? m->spec_armed.nplanes : 0;
  const size_t rowd = m ? spec_row_doubles(*m, np) : 0, nsh = m ? (size_t)np * m->nshell : 0;
  std::vector<double> rows(m && count > 0 && count <= m->ring.capacity ? (size_t)count * rowd : 0);  // (a count no ring can hold is refused below)
  if (int rc = ring_read(c, m ? &m->ring : nullptr, "ekpnp_spectrum_read", first, count, steps, times, shells ? rows.data() : nullptr)) return rc;
  for (int k = 0; k < count; ++k) {  // a row is [shells | peaks]
    const double* row = rows.data() + (size_t)k * rowd;
    std::memcpy(shells + (size_t)k * nsh, row, nsh * sizeof(double));
    if (peaks) std::memcpy(peaks + (size_t)k * np * 3, row + nsh, (size_t)np * 3 * sizeof(double));
  }
  return EKPNP_OK;
}

extern "C" int ekpnp_spectrum_save(ekpnp_ctx* ctx, const char* path) {
  NEEDCTX(ctx);
  if (!path) return fail(c, "NULL path");
  const ekpnp_spectrum_spec* spec = spectrum_armed_spec(c);
  if (!spec) return fail(c, "ekpnp_spectrum_save: no spectrum tracking was armed");
  const SpecState& m = *c.spectrum;
  int64_t rec = 0, dropped = 0;
  (void)ekpnp_spectrum_count(ctx, &rec, &dropped);
  const int n = (int)(rec - dropped);
  std::vector<int64_t> steps((size_t)n);
  std::vector<double> times((size_t)n), shells((size_t)n * spec->nplanes * m.nshell), peaks((size_t)n * spec->nplanes * 3);
  if (int rc = ekpnp_spectrum_read(ctx, 0, n, steps.data(), times.data(), shells.data(), peaks.data())) return rc;
  return spectrum_write_file(path, c.p, *spec, m.nshell, m.L, rec, dropped, n, steps.data(), times.data(), shells.data(), peaks.data(), c.err);
}
