// tracers.hip — Lagrangian tracers: one particle cloud per context, advected through the frozen fields on the device, with cell
// counts, displacement moments and their time series (include/ekpnp.h: ekpnp_tracers_*; no reference counterpart).
//
// Every other diagnostic is Eulerian.  Trajectories used to cost three ekpnp_get_field copies per sample (1.07 GB each at 512^3)
// and an interpolation loop on the host.  Here the cloud stays in device memory, structure of arrays, 56 B per particle:
//   k_tracers_advance<MOB>   one thread per particle, workgroups of 256.  The positions are loaded and stored coalesced; the nsub
//                            midpoint substeps run inside the kernel (the fields are frozen during the call).  An evaluation
//                            computes the 8-node stencil once and issues its 24 loads (MOB, mu != 0: 48, E beside u) before the
//                            first is used.  No LDS, no atomics.  Every index is clamped to the lattice before any load.
//   k_tracers_advance_brownian<MOB>   the same thread per particle, and after every midpoint substep a kick: one Philox4x32-10 call of
//                            (seed, the particle's ID, the cloud's epoch + the substep), three numbers in (-1, 1) times the kick
//                            lengths the host formed, x and y folded, z reflected at the plates.  The id array is read only when
//                            the cloud has one (a wave-uniform branch).  No LDS, no atomics, no scratch, no square root.
//   k_tracers_advance_absorbing<MOB>   the Brownian thread per particle with plates that ABSORB (a mask names them; the other reflects):
//                            a particle found on an absorbing plate stays there and its first arrival - the substep's number, the
//                            wall, x, y and the image counts - goes into the landing record, six arrays indexed by the particle's ID,
//                            so that exactly one thread ever touches an entry: no atomic.  A particle on such a plate at entry takes
//                            no substep and draws nothing: a wavefront of them leaves after the position loads.
//   k_tracers_advance_tangent<MOB>   the plain thread per particle (its positions, bit for bit) that also carries the flow-map gradient:
//                            F[9] and its exponent e, loaded once before the substeps and stored once after them from the stretch
//                            record ([9][n] doubles, then e: coalesced), F <- J F per substep with J the Jacobian of the midpoint
//                            substep, formed from the gradient of the interpolant - the SAME 24 / 48 loads, not one more - and
//                            renormalised by 2^+-64.  M1 = I + a G1 is formed before the second evaluation, so the two gradients are
//                            never both live.  No LDS, no atomics, no scratch.  k_stretch_begin makes the identity record and
//                            k_stretch_levels counts floor(log2 |F 2^e|^2) per level as k_landings_hist counts epochs.
//   k_landings_hist / k_landings_map<LDS>   the arrival-time histogram and the deposit map of a plate: the record read in id order,
//                            the counting of k_tracers_cells (uint32 counters in LDS, equal cells of a wavefront merged, 64-bit
//                            integer atomics to flush; a map beyond the LDS table counts with 64-bit global integer atomics)
//   k_tracers_seed           a thread per particle: Philox numbers (RANDOM) or three tables the host made (GRID)
//   k_tracers_cells<LDS>     counts per cell of a bx x by x bz partition: uint32 counters in LDS where the table fits 32 KB, flushed
//                            with 64-bit integer atomics; 64-bit global integer atomics otherwise.  Counts are integers: exact.
//   k_tracers_partials / k_tracers_finish   the 12 moments, the scheme of stats.hip over particles: runs of 4096 particles per
//                            workgroup, thread t adds t, t + 256, ... ascending, reduce.h's trees, partial sums in ascending order
// ekpnp_tracers_advance_host IS the definition of an advance, ekpnp_tracers_advance_brownian_host of a Brownian one,
// ekpnp_tracers_advance_absorbing_host of an absorbing one (all call tr_midpoint, the midpoint substep; the last two tr_kick),
// ekpnp_tracers_advance_tangent_host of a tangent one (tr_midpoint_tangent: tr_midpoint's operations on the positions, and J) and
// ekpnp_tracers_seed_host of a seed; the device leaves their bits by
// construction: stencil, interpolation, fold and step are ONE __host__ __device__ function each, the step constants are formed
// once on the host, and this object is built with -ffp-contract=off (csrc/Makefile, PINNED), so that neither side fuses a
// multiply-add.  The passive and the mu != 0 kernel are two instantiations of one template; mu alone chooses, not the shape.
// A gather is uncoalesced by nature: a GRID-seeded cloud starts in memory order, a stirred one does not (tools/time_tracers.py
// measures both cases).  ekpnp_tracers_sort puts a stirred cloud back into memory order (tools/time_tracers_sort.py measures it):
//   k_tracers_sort_keys      item[i] = key << 32 | i, the key being the linear index of the first node an advance loads
//   k_tracers_sort_hist / _scan / _scan_top / _scatter   four 8-bit passes of a stable LSD radix sort over the 64-bit items, for
//                            every lattice: a histogram per run of 4096 items, digit-major; its exclusive scan in two levels; a
//                            scatter whose ranks come from ballots and per-wave LDS counters - no atomic decides an order
//   k_tracers_sort_gather    the eight arrays and the ids through the final slot list, one array at a time through an 8-byte
//                            temporary per particle (the second item buffer, free after the last pass) and a copy back
// ekpnp_tracers_sort_host IS the definition of the order; it is unique, so the device equals it exactly.
// What a parcel sees on its way (ekpnp_tracers_sample*, ekpnp_tracks_*): the fields AT the particles, by the advance's own stencil
// and interpolation (tr_stencil, tr_load8, tr_interp; tr_sample is the per-particle function of host and device alike):
//   k_tracers_sample         a thread per particle: the stencil once, the named arrays in groups of at most three (24 loads in
//                            flight, q = c - cn counts two), coalesced stores to out[value][particle]
//   k_tracers_track_find     sorted clouds only: one pass over the ids with 16-byte loads, the ascending tag list in LDS, a binary
//                            search per id; the one thread that finds a tag stores its slot - no atomic
//   k_tracers_track_row      a thread per tag: x, y, z, wx, wy and the sampled values into the next row of the tracks' ring
// ekpnp_tracers_sample_host IS the definition of a sample.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ekpnp_internal.h"
#include "philox.h"
#include "reduce.h"
#include "ring.h"

using namespace ekpnp;

namespace ekpnp {

constexpr int TR_THREADS = 256;
constexpr int TR_PER_THREAD = 16;
constexpr int TR_CHUNK = TR_THREADS * TR_PER_THREAD;  // particles per workgroup of the moments
constexpr int TR_CELL_PER_THREAD = 32;                // particles per thread of the cell counts
constexpr int TR_LDS_CELLS = 8192;                    // counters (cells + 1) that fit the workgroup's 32 KB of LDS
constexpr int NM = EKPNP_NTRACER_MOMENTS;
constexpr const char* kSlabMsg = "tracers: slab contexts are not supported";
static const char* const kMomentNames[NM] = {"alive", "lost", "sum_dx", "sum_dy", "sum_dz", "sum_dx2", "sum_dy2", "sum_dz2", "sum_z", "sum_z2", "z_min", "z_max"};

struct TrFields {
  const double* u[3];  // ux, uy, uz [nz][ny][nx]
  const double* e[3];  // Ex, Ey, Ez (read only when mu != 0)
};
struct TrStep {
  double hx, hy, hz, ax, ay, az, mu;
  int nx, ny, nz, nsub;
};

// (int)v of a coordinate, clamped to 0 .. hi: inside the invariant this is (int)v itself; outside it is some index of the lattice
__host__ __device__ __forceinline__ int tr_index(double v, int hi) {
  int i = (v >= 0.0 && v < 2147483647.0) ? (int)v : 0;
  return i > hi ? hi : i;
}

// L(p, q, f): d = q - p; t = f*d; r = p + t
__host__ __device__ __forceinline__ double tr_lerp(double p, double q, double f) {
  const double d = q - p;
  const double t = f * d;
  return p + t;
}
// a[0..7] = the nodes (k0,j0,i0) (k0,j0,i1) (k0,j1,i0) (k0,j1,i1) (k1,j0,i0) (k1,j0,i1) (k1,j1,i0) (k1,j1,i1)
__host__ __device__ __forceinline__ double tr_interp(const double a[8], double fx, double fy, double fz) {
  const double a00 = tr_lerp(a[0], a[1], fx), a10 = tr_lerp(a[2], a[3], fx);
  const double a01 = tr_lerp(a[4], a[5], fx), a11 = tr_lerp(a[6], a[7], fx);
  const double b0 = tr_lerp(a00, a10, fy), b1 = tr_lerp(a01, a11, fy);
  return tr_lerp(b0, b1, fz);
}

// the stencil at (x, y, z), step 2 of an advance: the four row starts (k, j) * nx, the two columns and the three fractions; every
// index is clamped to the lattice, so whatever the position is, a load through it stays inside the arrays
struct TrStencil {
  long long r00, r10, r01, r11;
  int i0, i1;
  double fx, fy, fz;
};
__host__ __device__ __forceinline__ TrStencil tr_stencil(int nx, int ny, int nz, double x, double y, double z) {
  const int i0 = tr_index(x, nx - 1), j0 = tr_index(y, ny - 1), k0 = tr_index(z, nz - 2);
  const double fx = x - (double)i0, fy = y - (double)j0, fz = z - (double)k0;
  const int i1 = i0 + 1 == nx ? 0 : i0 + 1, j1 = j0 + 1 == ny ? 0 : j0 + 1, k1 = k0 + 1;
  const long long r00 = ((long long)k0 * ny + j0) * nx, r10 = ((long long)k0 * ny + j1) * nx;
  const long long r01 = ((long long)k1 * ny + j0) * nx, r11 = ((long long)k1 * ny + j1) * nx;
  return TrStencil{r00, r10, r01, r11, i0, i1, fx, fy, fz};
}
// the eight nodes of an array, in tr_interp's order
__host__ __device__ __forceinline__ void tr_load8(const double* p, const TrStencil& st, double a[8]) {
  a[0] = p[st.r00 + st.i0]; a[1] = p[st.r00 + st.i1];
  a[2] = p[st.r10 + st.i0]; a[3] = p[st.r10 + st.i1];
  a[4] = p[st.r01 + st.i0]; a[5] = p[st.r01 + st.i1];
  a[6] = p[st.r11 + st.i0]; a[7] = p[st.r11 + st.i1];
}

// w[c] = u_c (+ mu E_c) at (x, y, z): the stencil once, every load before the first use
template <bool MOB>
__host__ __device__ __forceinline__ void tr_velocity(const TrFields& f, const TrStep& s, double x, double y, double z, double w[3]) {
  const TrStencil st = tr_stencil(s.nx, s.ny, s.nz, x, y, z);
  constexpr int NA = MOB ? 6 : 3;
  double a[NA][8];
#pragma unroll
  for (int q = 0; q < NA; ++q) tr_load8(q < 3 ? f.u[q] : f.e[q - 3], st, a[q]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    w[c] = tr_interp(a[c], st.fx, st.fy, st.fz);
    if constexpr (MOB) {
      const double t = s.mu * tr_interp(a[3 + c], st.fx, st.fy, st.fz);
      w[c] = w[c] + t;
    }
  }
}

__host__ __device__ __forceinline__ bool tr_lost(double x, double y, double z) { return x != x || y != y || z != z; }

// ---- sampling the fields at a particle (include/ekpnp.h: ekpnp_tracers_sample_host IS the definition) -------------------------
constexpr int TR_MAXV = EKPNP_TRACERS_MAX_VALUES;
constexpr int TR_GROUP = 3;  // arrays loaded before the first use: 24 loads in flight, the shape of a passive evaluation

// A group of at most TR_GROUP arrays and what is made of them: entry e is nothing (TR_OP_NONE: the second array of a Q, or past
// the group's end), the value of array e (TR_OP_VALUE), or q from the arrays e (c) and e + 1 (cn) (TR_OP_Q); slot[e] is the place
// of the result among the call's values.
enum { TR_OP_NONE = 0, TR_OP_VALUE = 1, TR_OP_Q = 2 };
struct TrGroup {
  const double* p[TR_GROUP];
  int8_t op[TR_GROUP], slot[TR_GROUP];
  int16_t narr;
};
struct TrSample {
  TrGroup g[TR_MAXV];  // a group holds at least one value: never more groups than values
  int ngroups, nvalues;
  int nx, ny, nz;
};

// every value of the call at (x, y, z) into out[slot * vstride]: NaN for a lost particle (nothing is read for it), else the
// stencil ONCE and group after group: all loads of a group before its first use, then v = L(L(L x) y) z of each value - for q
// of the eight differences d_m = c_m - cn_m, each a subtraction of its own
__host__ __device__ __forceinline__ void tr_sample(const TrSample& a, double x, double y, double z, double* out, long long vstride) {
  if (tr_lost(x, y, z)) {
    for (int v = 0; v < a.nvalues; ++v) out[v * vstride] = NAN;
    return;
  }
  const TrStencil st = tr_stencil(a.nx, a.ny, a.nz, x, y, z);
  for (int g = 0; g < a.ngroups; ++g) {
    const TrGroup& G = a.g[g];
    double v[TR_GROUP][8];
#pragma unroll
    for (int q = 0; q < TR_GROUP; ++q)
      if (q < G.narr) tr_load8(G.p[q], st, v[q]);
#pragma unroll
    for (int q = 0; q < TR_GROUP; ++q) {
      if (G.op[q] == TR_OP_VALUE) {
        out[G.slot[q] * vstride] = tr_interp(v[q], st.fx, st.fy, st.fz);
      } else if (q + 1 < TR_GROUP && G.op[q] == TR_OP_Q) {
        double d[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) d[m] = v[q][m] - v[q + 1 < TR_GROUP ? q + 1 : q][m];
        out[G.slot[q] * vstride] = tr_interp(d, st.fx, st.fy, st.fz);
      }
    }
  }
}

// the fold of a periodic coordinate (include/ekpnp.h, step 6); false: the particle is lost
__host__ __device__ __forceinline__ bool tr_fold(double& x, double n, int& w) {
  if (x >= n) { x = x - n; w += 1; }
  else if (x < 0.0) { x = x + n; w -= 1; }
  if (x >= n) { x = x - n; w += 1; }
  return x >= 0.0 && x < n;
}
// z between the plates; false (NaN, Inf): the particle is lost
__host__ __device__ __forceinline__ bool tr_fold_z(double& z, double top) {
  if (!(z >= -1.7976931348623157e308 && z <= 1.7976931348623157e308)) return false;
  if (z < 0.0) z = 0.0;
  if (z > top) z = top;
  return true;
}

// one midpoint substep (include/ekpnp.h, step 5) of a particle that is not lost: true, and x, y, z and the image counts are the
// new ones; false: the particle is lost and nothing was written
template <bool MOB>
__host__ __device__ __forceinline__ bool tr_midpoint(const TrFields& f, const TrStep& s, double px, double py, double top, double& x, double& y, double& z, int& wx, int& wy) {
  double w[3];
  tr_velocity<MOB>(f, s, x, y, z, w);
  double t = s.ax * w[0];
  double x1 = x + t;
  t = s.ay * w[1];
  double y1 = y + t;
  t = s.az * w[2];
  double z1 = z + t;
  int none = 0;
  bool ok = tr_fold(x1, px, none);
  ok = tr_fold(y1, py, none) && ok;
  ok = tr_fold_z(z1, top) && ok;
  if (ok) {
    tr_velocity<MOB>(f, s, x1, y1, z1, w);
    t = s.hx * w[0];
    x1 = x + t;
    t = s.hy * w[1];
    y1 = y + t;
    t = s.hz * w[2];
    z1 = z + t;
    int nwx = wx, nwy = wy;
    ok = tr_fold(x1, px, nwx);
    ok = tr_fold(y1, py, nwy) && ok;
    ok = tr_fold_z(z1, top) && ok;
    if (ok) { x = x1; y = y1; z = z1; wx = nwx; wy = nwy; }
  }
  return ok;
}

// nsub midpoint substeps of one particle that is not lost on entry
template <bool MOB>
__host__ __device__ __forceinline__ void tr_advance(const TrFields& f, const TrStep& s, double& x, double& y, double& z, int& wx, int& wy) {
  const double px = (double)s.nx, py = (double)s.ny, top = (double)(s.nz - 1);
  for (int it = 0; it < s.nsub; ++it) {
    const bool ok = tr_midpoint<MOB>(f, s, px, py, top, x, y, z, wx, wy);
    if (!ok) {  // lost: the image counts stay what they were
      x = y = z = NAN;
      return;
    }
  }
}

// ---- the flow-map gradient (include/ekpnp.h: ekpnp_tracers_advance_tangent_host IS the definition) -----------------------------
// tr_interp's value (its bits) and the three derivatives per cell of the interpolant, from the same eight nodes
__host__ __device__ __forceinline__ double tr_interp_grad(const double a[8], double fx, double fy, double fz, double g[3]) {
  const double a00 = tr_lerp(a[0], a[1], fx), a10 = tr_lerp(a[2], a[3], fx);
  const double a01 = tr_lerp(a[4], a[5], fx), a11 = tr_lerp(a[6], a[7], fx);
  const double b0 = tr_lerp(a00, a10, fy), b1 = tr_lerp(a01, a11, fy);
  const double d0 = a[1] - a[0], d1 = a[3] - a[2], d2 = a[5] - a[4], d3 = a[7] - a[6];
  g[0] = tr_lerp(tr_lerp(d0, d1, fy), tr_lerp(d2, d3, fy), fz);
  const double e0 = a10 - a00, e1 = a11 - a01;
  g[1] = tr_lerp(e0, e1, fz);
  g[2] = b1 - b0;
  return tr_lerp(b0, b1, fz);
}

// tr_velocity and beside it G[3c + r] = the derivative of w[c] along r: the stencil once, every load before the first use
template <bool MOB>
__host__ __device__ __forceinline__ void tr_velocity_grad(const TrFields& f, const TrStep& s, double x, double y, double z, double w[3], double G[9]) {
  const TrStencil st = tr_stencil(s.nx, s.ny, s.nz, x, y, z);
  constexpr int NA = MOB ? 6 : 3;
  double a[NA][8];
#pragma unroll
  for (int q = 0; q < NA; ++q) tr_load8(q < 3 ? f.u[q] : f.e[q - 3], st, a[q]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    w[c] = tr_interp_grad(a[c], st.fx, st.fy, st.fz, G + 3 * c);
    if constexpr (MOB) {
      double ge[3];
      const double t = s.mu * tr_interp_grad(a[3 + c], st.fx, st.fy, st.fz, ge);
      w[c] = w[c] + t;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double tg = s.mu * ge[r];
        G[3 * c + r] = G[3 * c + r] + tg;
      }
    }
  }
}

// tr_midpoint (its positions, image counts and verdict, operation by operation) and F <- J F, J the Jacobian of the substep.  M1 is
// formed before the second evaluation: the two gradients are never both live.  false: the particle is lost, F is not written.
template <bool MOB>
__host__ __device__ __forceinline__ bool tr_midpoint_tangent(const TrFields& f, const TrStep& s, double px, double py, double top, double& x, double& y, double& z, int& wx,
                                                             int& wy, double F[9]) {
  double w[3], G[9], M[9];
  tr_velocity_grad<MOB>(f, s, x, y, z, w, G);
  double t = s.ax * w[0];
  double x1 = x + t;
  t = s.ay * w[1];
  double y1 = y + t;
  t = s.az * w[2];
  double z1 = z + t;
  const double a[3] = {s.ax, s.ay, s.az}, h[3] = {s.hx, s.hy, s.hz};
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double m = a[q] * G[3 * q + r];
      M[3 * q + r] = q == r ? 1.0 + m : m;
    }
  int none = 0;
  bool ok = tr_fold(x1, px, none);
  ok = tr_fold(y1, py, none) && ok;
  ok = tr_fold_z(z1, top) && ok;
  if (ok) {
    tr_velocity_grad<MOB>(f, s, x1, y1, z1, w, G);
    t = s.hx * w[0];
    x1 = x + t;
    t = s.hy * w[1];
    y1 = y + t;
    t = s.hz * w[2];
    z1 = z + t;
    int nwx = wx, nwy = wy;
    ok = tr_fold(x1, px, nwx);
    ok = tr_fold(y1, py, nwy) && ok;
    ok = tr_fold_z(z1, top) && ok;
    if (ok) {
      x = x1; y = y1; z = z1; wx = nwx; wy = nwy;
      double J[9];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double t0 = G[3 * c] * M[r], t1 = G[3 * c + 1] * M[3 + r], t2 = G[3 * c + 2] * M[6 + r];
          const double u01 = t0 + t1;
          const double S = u01 + t2;
          const double j = h[c] * S;
          J[3 * c + r] = c == r ? 1.0 + j : j;
        }
      double N[9];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double t0 = J[3 * c] * F[r], t1 = J[3 * c + 1] * F[3 + r], t2 = J[3 * c + 2] * F[6 + r];
          const double u01 = t0 + t1;
          N[3 * c + r] = u01 + t2;
        }
#pragma unroll
      for (int q = 0; q < 9; ++q) F[q] = N[q];
    }
  }
  return ok;
}

// the renormalisation after a substep: the largest |F[q]| kept inside [2^-64, 2^64) by exact multiplications, e counts them
__host__ __device__ __forceinline__ void tr_renormalise(double F[9], int& e) {
  double m = 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const double a = F[q] < 0.0 ? 0.0 - F[q] : F[q];
    if (a > m) m = a;
  }
  if (m >= 0x1.0p64) {
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = F[q] * 0x1.0p-64;
    e += 64;
  } else if (m > 0.0 && m < 0x1.0p-64) {
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = F[q] * 0x1.0p64;
    e -= 64;
  }
}

// nsub tangent substeps of one particle that is not lost on entry
template <bool MOB>
__host__ __device__ __forceinline__ void tr_advance_tangent(const TrFields& f, const TrStep& s, double& x, double& y, double& z, int& wx, int& wy, double F[9], int& e) {
  const double px = (double)s.nx, py = (double)s.ny, top = (double)(s.nz - 1);
  for (int it = 0; it < s.nsub; ++it) {
    const bool ok = tr_midpoint_tangent<MOB>(f, s, px, py, top, x, y, z, wx, wy, F);
    if (!ok) {  // lost: the image counts and e stay what they were
      x = y = z = NAN;
#pragma unroll
      for (int q = 0; q < 9; ++q) F[q] = NAN;
      return;
    }
    tr_renormalise(F, e);
  }
}

// the level of a particle (include/ekpnp.h: ekpnp_stretch_level): floor(log2 |F 2^e|^2), the exponent from trC's bit pattern
constexpr int32_t TR_NO_LEVEL = INT32_MIN;
__host__ __device__ __forceinline__ int32_t tr_stretch_level(const double F[9], int32_t e) {
  double trc = F[0] * F[0];
#pragma unroll
  for (int q = 1; q < 9; ++q) {
    const double p = F[q] * F[q];
    trc = trc + p;
  }
  if (trc != trc || trc == 0.0) return TR_NO_LEVEL;
  int bias = 0;
  union { double d; uint64_t u; } v;
  v.d = trc;
  if (((v.u >> 52) & 0x7ffu) == 0) {  // subnormal: scaled into the normal range, exactly
    v.d = trc * 0x1.0p54;
    bias = -54;
  }
  const int E = (int)((v.u >> 52) & 0x7ffu) - 1022 + bias;  // trC = f * 2^E, 0.5 <= f < 1
  const long long l = 2ll * (long long)e + (long long)E - 1ll;
  return l <= (long long)INT32_MIN ? INT32_MIN + 1 : l > (long long)INT32_MAX ? INT32_MAX : (int32_t)l;
}

// ---- Brownian substeps (include/ekpnp.h: ekpnp_tracers_advance_brownian_host IS the definition) -------------------------------
// the noise of a call: the kick lengths in cells, formed once on the host (the device takes no square root), the seed, and the
// epoch of the call's first substep
struct TrNoise {
  double kx, ky, kz;
  uint64_t seed;
  int64_t epoch;
};
constexpr uint32_t TR_KICK_TAG = 0x80000000u;  // the fourth counter word of a kick is never 0, which is seed_uniform's

// r[0..2] of (seed, id, epoch): one Philox call; ((double)(int32)word + 0.5) * 2^-31 is exact, symmetric, never 0, in (-1, 1)
__host__ __device__ __forceinline__ void tr_kick(uint64_t seed, int64_t id, int64_t epoch, double r[3]) {
  const uint64_t i = (uint64_t)id, e = (uint64_t)epoch;
  uint32_t c[4] = {(uint32_t)(i & 0xffffffffu), (uint32_t)(e & 0xffffffffu), (uint32_t)(e >> 32), TR_KICK_TAG | (uint32_t)(i >> 32)};
  philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = (double)(int32_t)c[a];
    const double s = v + 0.5;
    r[a] = s * 0x1.0p-31;
  }
}

// z after a kick, reflected at the plates and then held by them (a kick longer than the channel); false (NaN, Inf): lost
__host__ __device__ __forceinline__ bool tr_reflect_z(double& z, double top) {
  if (z < 0.0) z = 0.0 - z;
  if (z > top) {
    const double d = z - top;
    z = top - d;
  }
  return tr_fold_z(z, top);
}

// nsub Brownian substeps of the particle `id`, not lost on entry: the midpoint substep, the kick of (seed, id, epoch + it), the
// fold of x and y with their image counts, the reflection of z
template <bool MOB>
__host__ __device__ __forceinline__ void tr_advance_brownian(const TrFields& f, const TrStep& s, const TrNoise& q, int64_t id, double& x, double& y, double& z,
                                                             int& wx, int& wy) {
  const double px = (double)s.nx, py = (double)s.ny, top = (double)(s.nz - 1);
  for (int it = 0; it < s.nsub; ++it) {
    const int owx = wx, owy = wy;
    bool ok = tr_midpoint<MOB>(f, s, px, py, top, x, y, z, wx, wy);
    if (ok) {
      double r[3];
      tr_kick(q.seed, id, q.epoch + (int64_t)it, r);
      double t = q.kx * r[0];
      x = x + t;
      t = q.ky * r[1];
      y = y + t;
      t = q.kz * r[2];
      z = z + t;
      ok = tr_fold(x, px, wx);
      ok = tr_fold(y, py, wy) && ok;
      ok = tr_reflect_z(z, top) && ok;
    }
    if (!ok) {  // lost: the image counts stay what they were before the substep
      x = y = z = NAN;
      wx = owx;
      wy = owy;
      return;
    }
  }
}

// ---- absorbing plates (include/ekpnp.h: ekpnp_tracers_advance_absorbing_host IS the definition) ------------------------------
// the landing record: six arrays [n] indexed by the particle's ID, one allocation in the order of the record's file
struct TrLand {
  int64_t* epoch;  // -1: not landed
  double *x, *y;   // NaN: not landed
  int32_t *wall, *wx, *wy;
};

// the absorbing plate a height lies on: 1 (bottom), 2 (top), 0: none
__host__ __device__ __forceinline__ int tr_on_plate(int walls, double z, double top) {
  if ((walls & 1) && z <= 0.0) return 1;
  if ((walls & 2) && z >= top) return 2;
  return 0;
}

// z after a kick: an absorbing plate keeps what went through it, the other reflects it (tr_reflect_z); then the hold; false: lost
__host__ __device__ __forceinline__ bool tr_absorb_z(double& z, double top, int walls) {
  if (!(z >= -1.7976931348623157e308 && z <= 1.7976931348623157e308)) return false;
  if (z < 0.0) z = (walls & 1) ? 0.0 : 0.0 - z;
  if (z > top) {
    if (walls & 2) {
      z = top;
    } else {
      const double d = z - top;
      z = top - d;
    }
  }
  return tr_fold_z(z, top);
}

// nsub absorbing substeps of the particle `id`, neither lost nor on an absorbing plate on entry: tr_advance_brownian until the
// particle is found on an absorbing plate - after the midpoint substep (drift into the wall: no kick follows) or after the kick.
// Returns that wall (0: none) and in `at` the substep; x, y, z and the image counts are then the landing place.
template <bool MOB>
__host__ __device__ __forceinline__ int tr_advance_absorbing(const TrFields& f, const TrStep& s, const TrNoise& q, int walls, int64_t id, double& x, double& y,
                                                             double& z, int& wx, int& wy, int& at) {
  const double px = (double)s.nx, py = (double)s.ny, top = (double)(s.nz - 1);
  for (int it = 0; it < s.nsub; ++it) {
    const int owx = wx, owy = wy;
    bool ok = tr_midpoint<MOB>(f, s, px, py, top, x, y, z, wx, wy);
    int wall = 0;
    if (ok) {
      wall = tr_on_plate(walls, z, top);
      if (!wall) {
        double r[3];
        tr_kick(q.seed, id, q.epoch + (int64_t)it, r);
        double t = q.kx * r[0];
        x = x + t;
        t = q.ky * r[1];
        y = y + t;
        t = q.kz * r[2];
        z = z + t;
        ok = tr_fold(x, px, wx);
        ok = tr_fold(y, py, wy) && ok;
        ok = tr_absorb_z(z, top, walls) && ok;
        if (ok) wall = tr_on_plate(walls, z, top);
      }
    }
    if (!ok) {  // lost: the image counts stay what they were before the substep, and no landing is recorded
      x = y = z = NAN;
      wx = owx;
      wy = owy;
      return 0;
    }
    if (wall) {
      at = it;
      return wall;
    }
  }
  return 0;
}

// the cell of an arrival-time histogram (include/ekpnp.h: ekpnp_landings_bin), 64-bit integer arithmetic; e0 >= 0, width >= 1
__host__ __device__ __forceinline__ int tr_land_bin(int64_t e0, int64_t width, int nbins, int64_t epoch) {
  if (epoch < e0) return 0;
  const int64_t d = (epoch - e0) / width;
  return d >= (int64_t)nbins ? nbins + 1 : 1 + (int)d;
}

// the cell of a position (include/ekpnp.h: ekpnp_tracers_cell), -1 for a lost particle
__host__ __device__ __forceinline__ int tr_cell(int nx, int ny, int nz, int bx, int by, int bz, double x, double y, double z) {
  if (tr_lost(x, y, z)) return -1;
  const int i0 = tr_index(x, nx - 1), j0 = tr_index(y, ny - 1), k0 = tr_index(z, nz - 2);
  const int cx = (int)(((long long)i0 * bx) / nx), cy = (int)(((long long)j0 * by) / ny), cz = (int)(((long long)k0 * bz) / (nz - 1));
  return (cz * by + cy) * bx + cx;
}

// a RANDOM start coordinate: r in [-1, 1) -> u in [0, 1) (exact) -> the box; t = hi - lo
__host__ __device__ __forceinline__ double tr_seed_random(uint64_t seed, uint64_t p, int axis, double lo, double hi, double t, double period) {
  const double r = seed_uniform(seed, p, 16 + axis);
  const double h = 0.5 * r;
  const double u = h + 0.5;
  const double s = u * t;
  const double v = lo + s;
  return (v >= hi || v >= period) ? lo : v;
}

struct TrCloud {
  double *x, *y, *z, *x0, *y0, *z0;
  int32_t *wx, *wy;
  long long n;
};

template <bool MOB>
__global__ void __launch_bounds__(TR_THREADS) k_tracers_advance(TrFields f, TrStep s, TrCloud c) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= c.n) return;
  double x = c.x[i], y = c.y[i], z = c.z[i];
  if (tr_lost(x, y, z)) return;  // nothing is read, nothing is written
  int wx = c.wx[i], wy = c.wy[i];
  tr_advance<MOB>(f, s, x, y, z, wx, wy);
  c.x[i] = x;
  c.y[i] = y;
  c.z[i] = z;
  c.wx[i] = wx;
  c.wy[i] = wy;
}

// ids == null: the cloud was never sorted and the id of a particle is its slot (a kernel argument: the branch is wave-uniform)
template <bool MOB>
__global__ void __launch_bounds__(TR_THREADS) k_tracers_advance_brownian(TrFields f, TrStep s, TrNoise q, TrCloud c, const int32_t* __restrict__ ids) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= c.n) return;
  double x = c.x[i], y = c.y[i], z = c.z[i];
  if (tr_lost(x, y, z)) return;  // nothing is read, nothing is written
  const int64_t id = ids ? (int64_t)ids[i] : (int64_t)i;
  int wx = c.wx[i], wy = c.wy[i];
  tr_advance_brownian<MOB>(f, s, q, id, x, y, z, wx, wy);
  c.x[i] = x;
  c.y[i] = y;
  c.z[i] = z;
  c.wx[i] = wx;
  c.wy[i] = wy;
}

// A particle on an absorbing plate at entry (stuck) reads its record entry and, if that is empty, its image counts; everybody else
// is a Brownian thread that may end early.  The record is indexed by id and the ids are a permutation: one thread per entry.
template <bool MOB>
__global__ void __launch_bounds__(TR_THREADS) k_tracers_advance_absorbing(TrFields f, TrStep s, TrNoise q, int walls, TrCloud c, const int32_t* __restrict__ ids, TrLand L) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= c.n) return;
  double x = c.x[i], y = c.y[i], z = c.z[i];
  if (tr_lost(x, y, z)) return;  // nothing is read, nothing is written
  int wall = tr_on_plate(walls, z, (double)(s.nz - 1));
  const int64_t id = ids ? (int64_t)ids[i] : (int64_t)i;
  if (id < 0 || id >= c.n) return;  // (a permutation of ids never comes here)
  int64_t when = q.epoch;
  int wx, wy;
  if (wall) {  // stuck: no substep, no draw, no store to the cloud
    if (L.epoch[id] >= 0) return;
    wx = c.wx[i];
    wy = c.wy[i];
  } else {
    wx = c.wx[i];
    wy = c.wy[i];
    int at = 0;
    wall = tr_advance_absorbing<MOB>(f, s, q, walls, id, x, y, z, wx, wy, at);
    c.x[i] = x;
    c.y[i] = y;
    c.z[i] = z;
    c.wx[i] = wx;
    c.wy[i] = wy;
    if (!wall) return;
    when = q.epoch + (int64_t)at + 1;
    if (L.epoch[id] >= 0) return;  // a FIRST-passage record
  }
  L.epoch[id] = when;
  L.wall[id] = wall;
  L.x[id] = x;
  L.y[id] = y;
  L.wx[id] = wx;
  L.wy[id] = wy;
}

// the stretch record in slot order: F[q][n] (entry q of the particle in slot i at F[q * n + i]) and e[n]
struct TrStretch {
  double* F;
  int32_t* e;
};

// F and e are loaded once before the substeps and stored once after them: the loads and stores of a wavefront are coalesced
template <bool MOB>
__global__ void __launch_bounds__(TR_THREADS) k_tracers_advance_tangent(TrFields f, TrStep s, TrCloud c, TrStretch r) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= c.n) return;
  double x = c.x[i], y = c.y[i], z = c.z[i];
  if (tr_lost(x, y, z)) return;  // nothing is read, nothing is written
  int wx = c.wx[i], wy = c.wy[i];
  double F[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) F[q] = r.F[(long long)q * c.n + i];
  int e = r.e[i];
  tr_advance_tangent<MOB>(f, s, x, y, z, wx, wy, F, e);
  c.x[i] = x;
  c.y[i] = y;
  c.z[i] = z;
  c.wx[i] = wx;
  c.wy[i] = wy;
#pragma unroll
  for (int q = 0; q < 9; ++q) r.F[(long long)q * c.n + i] = F[q];
  r.e[i] = e;
}

// a new record: F = the identity and e = 0; F = NaN for a particle that is already lost
__global__ void __launch_bounds__(TR_THREADS) k_stretch_begin(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z, long long n, TrStretch r) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool lost = tr_lost(x[i], y[i], z[i]);
#pragma unroll
  for (int q = 0; q < 9; ++q) r.F[(long long)q * n + i] = lost ? NAN : (q % 4 == 0 ? 1.0 : 0.0);
  r.e[i] = 0;
}

// out[v][i] = value v at the particle in slot i: the stores of a wavefront are coalesced
__global__ void __launch_bounds__(TR_THREADS) k_tracers_sample(TrSample a, const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                               long long n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n) return;
  tr_sample(a, x[i], y[i], z[i], out + i, n);
}

// The tag tables of a track ring (its header): the ids as given, the ids ascending, the place each of those had in the given
// order, and the slot found for each place.  All [ntags]; the first three are written by the host when the ring is armed.
struct TrTags {
  const int32_t *ids, *sorted, *place;
  int32_t* slot;
  int ntags;
};
constexpr int TK_IDS = 4;  // ids per thread of the find: one 16-byte load

// slot[place of id[s]] = s for every slot s whose id is tagged: one pass over the ids, the ascending tag list in LDS, a binary
// search per id.  The ids are a permutation, so exactly one thread finds each tag: no atomic, no race decides anything.
__global__ void __launch_bounds__(TR_THREADS) k_tracers_track_find(const int32_t* __restrict__ ids, long long n, TrTags t) {
  __shared__ int32_t key[EKPNP_TRACERS_MAX_TRACKS], place[EKPNP_TRACERS_MAX_TRACKS];
  for (int k = threadIdx.x; k < t.ntags; k += TR_THREADS) {
    key[k] = t.sorted[k];
    place[k] = t.place[k];
  }
  __syncthreads();
  const long long base = ((long long)blockIdx.x * TR_THREADS + threadIdx.x) * TK_IDS;
  if (base >= n) return;
  int32_t v[TK_IDS] = {-1, -1, -1, -1};  // (no tag is negative)
  if (base + TK_IDS <= n) {
    const int4 q = *(const int4*)(ids + base);  // base is a multiple of 4 and the array starts an allocation: aligned
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int k = 0; base + k < n; ++k) v[k] = ids[base + k];
  }
#pragma unroll
  for (int k = 0; k < TK_IDS; ++k) {
    int lo = 0, hi = t.ntags;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] < v[k]) lo = mid + 1;
      else hi = mid;
    }
    if (lo < t.ntags && key[lo] == v[k]) {
      const int at = place[lo];
      if (at >= 0 && at < t.ntags) t.slot[at] = (int32_t)(base + k);
    }
  }
}

// row[tag] = x, y, z, (double)wx, (double)wy and the sampled values of the tagged particle: the bits ekpnp_tracers_get and
// ekpnp_tracers_sample give for it.  slots == null: the cloud was never sorted and the slot of a particle is its id.
__global__ void __launch_bounds__(TR_THREADS) k_tracers_track_row(TrSample a, TrCloud c, TrTags t, const int32_t* __restrict__ slots, double* __restrict__ row) {
  const int tag = blockIdx.x * TR_THREADS + threadIdx.x;
  if (tag >= t.ntags) return;
  double* r = row + (size_t)tag * (size_t)(5 + a.nvalues);
  const long long s = slots ? slots[tag] : t.ids[tag];
  if (s < 0 || s >= c.n) {  // (a checked spec and a permutation of ids never come here)
    for (int q = 0; q < 5 + a.nvalues; ++q) r[q] = NAN;
    return;
  }
  const double x = c.x[s], y = c.y[s], z = c.z[s];
  r[0] = x;
  r[1] = y;
  r[2] = z;
  r[3] = (double)c.wx[s];
  r[4] = (double)c.wy[s];
  tr_sample(a, x, y, z, r + 5, 1);
}

struct TrSeedArgs {
  double lo[3], hi[3], t[3], period[3];  // t = hi - lo; period: nx, ny, +Inf
  uint64_t seed;
  const double* tab;                     // GRID: [gx | gy | gz] coordinates
  int mode, gx, gy, gz;
};

__global__ void __launch_bounds__(TR_THREADS) k_tracers_seed(TrSeedArgs a, TrCloud c) {
  const long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (p >= c.n) return;
  double v[3];
  if (a.mode == EKPNP_TRACERS_GRID) {
    const long long row = p / a.gx;
    const int i = (int)(p - row * a.gx), k = (int)(row / a.gy), j = (int)(row - (long long)k * a.gy);
    v[0] = a.tab[i];
    v[1] = a.tab[a.gx + j];
    v[2] = a.tab[a.gx + a.gy + (k < a.gz ? k : a.gz - 1)];
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = tr_seed_random(a.seed, (uint64_t)p, q, a.lo[q], a.hi[q], a.t[q], a.period[q]);
  }
  c.x[p] = v[0]; c.y[p] = v[1]; c.z[p] = v[2];
  c.x0[p] = v[0]; c.y0[p] = v[1]; c.z0[p] = v[2];
  c.wx[p] = 0;
  c.wy[p] = 0;
}

// the lanes that agree with the wavefront's first lane add their number at once (hist.hip: hist_add); cell < 0: nothing to add
__device__ __forceinline__ void tr_count_add(unsigned* cnt, int cell) {
  const int lead = __builtin_amdgcn_readfirstlane(cell);
  const bool same = cell == lead;
  const unsigned long long m = __ballot(same);
  if (same) {
    if (lead >= 0 && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&cnt[lead], (unsigned)__popcll(m));
  } else if (cell >= 0) {
    atomicAdd(&cnt[cell], 1u);
  }
}

// total[cell] += the workgroup's particles in it; total[cells] counts the lost ones (zeroed by the host's memset before)
template <bool LDS>
__global__ void __launch_bounds__(TR_THREADS) k_tracers_cells(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z, long long n,
                                                              int nx, int ny, int nz, int bx, int by, int bz, int cells, unsigned long long* __restrict__ total) {
  extern __shared__ unsigned tr_cnt[];
  if constexpr (LDS) {
    for (int i = threadIdx.x; i <= cells; i += TR_THREADS) tr_cnt[i] = 0u;
    __syncthreads();
  }
  const long long first = (long long)blockIdx.x * (TR_THREADS * TR_CELL_PER_THREAD) + threadIdx.x;
  for (int k0 = 0; k0 < TR_CELL_PER_THREAD; k0 += 8) {
    double px[8], py[8], pz[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      const bool in = i < n;
      px[k] = in ? x[i] : 0.0;
      py[k] = in ? y[i] : 0.0;
      pz[k] = in ? z[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      int cell = tr_cell(nx, ny, nz, bx, by, bz, px[k], py[k], pz[k]);
      if (cell < 0) cell = cells;
      if (i >= n) cell = -1;
      if constexpr (LDS) tr_count_add(tr_cnt, cell);
      else if (cell >= 0) atomicAdd(&total[cell], 1ull);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i <= cells; i += TR_THREADS) {
      const unsigned v = tr_cnt[i];
      if (v) atomicAdd(&total[i], (unsigned long long)v);
    }
  }
}

// total[cell of ekpnp_landings_bin] += the workgroup's landings on a wall of the mask; total[nbins + 2] counts everybody else.
// The table has at most 4099 counters: it always fits the LDS.  12 B per particle, in id order.
__global__ void __launch_bounds__(TR_THREADS) k_landings_hist(const int64_t* __restrict__ epoch, const int32_t* __restrict__ wall, long long n, int walls, int64_t e0,
                                                              int64_t width, int nbins, unsigned long long* __restrict__ total) {
  extern __shared__ unsigned tr_cnt[];
  const int cells = nbins + 2;
  for (int i = threadIdx.x; i <= cells; i += TR_THREADS) tr_cnt[i] = 0u;
  __syncthreads();
  const long long first = (long long)blockIdx.x * (TR_THREADS * TR_CELL_PER_THREAD) + threadIdx.x;
  for (int k0 = 0; k0 < TR_CELL_PER_THREAD; k0 += 8) {
    int64_t e[8];
    int32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      const bool in = i < n;
      e[k] = in ? epoch[i] : -1;
      w[k] = in ? wall[i] : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      const bool counted = (w[k] == 1 || w[k] == 2) && (walls & w[k]) && e[k] >= 0;
      int cell = counted ? tr_land_bin(e0, width, nbins, e[k]) : cells;
      if (i >= n) cell = -1;
      tr_count_add(tr_cnt, cell);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= cells; i += TR_THREADS) {
    const unsigned v = tr_cnt[i];
    if (v) atomicAdd(&total[i], (unsigned long long)v);
  }
}

constexpr int TR_LEVEL_BATCH = 4;  // particles of a thread in flight: 36 doubles and 4 int32

// total[cell of the level] += the workgroup's particles: cell 0 below l_lo, 1 + k for level l_lo + k, nlevels + 1 at or above
// l_lo + nlevels, nlevels + 2 for those without a level.  At most 4099 counters: the table always fits the LDS.  76 B per particle.
__global__ void __launch_bounds__(TR_THREADS) k_stretch_levels(TrStretch r, long long n, int l_lo, int nlevels, unsigned long long* __restrict__ total) {
  extern __shared__ unsigned tr_cnt[];
  const int cells = nlevels + 2;
  for (int i = threadIdx.x; i <= cells; i += TR_THREADS) tr_cnt[i] = 0u;
  __syncthreads();
  const long long first = (long long)blockIdx.x * (TR_THREADS * TR_CELL_PER_THREAD) + threadIdx.x;
  for (int k0 = 0; k0 < TR_CELL_PER_THREAD; k0 += TR_LEVEL_BATCH) {
    double F[TR_LEVEL_BATCH][9];
    int32_t e[TR_LEVEL_BATCH];
#pragma unroll
    for (int k = 0; k < TR_LEVEL_BATCH; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      const bool in = i < n;
#pragma unroll
      for (int q = 0; q < 9; ++q) F[k][q] = in ? r.F[(long long)q * n + i] : 0.0;
      e[k] = in ? r.e[i] : 0;
    }
#pragma unroll
    for (int k = 0; k < TR_LEVEL_BATCH; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      const int32_t level = tr_stretch_level(F[k], e[k]);
      const long long d = (long long)level - (long long)l_lo;
      int cell = level == TR_NO_LEVEL ? cells : d < 0 ? 0 : d >= (long long)nlevels ? nlevels + 1 : 1 + (int)d;
      if (i >= n) cell = -1;
      tr_count_add(tr_cnt, cell);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= cells; i += TR_THREADS) {
    const unsigned v = tr_cnt[i];
    if (v) atomicAdd(&total[i], (unsigned long long)v);
  }
}

// total[cell of ekpnp_tracers_cell(bx, by, 1)] += the workgroup's landings on `wall` with e_lo <= epoch <= e_hi; total[cells] counts
// everybody else.  28 B per particle, in id order.
template <bool LDS>
__global__ void __launch_bounds__(TR_THREADS) k_landings_map(TrLand L, long long n, int wall, int64_t e_lo, int64_t e_hi, int nx, int ny, int nz, int bx, int by,
                                                             int cells, unsigned long long* __restrict__ total) {
  extern __shared__ unsigned tr_cnt[];
  if constexpr (LDS) {
    for (int i = threadIdx.x; i <= cells; i += TR_THREADS) tr_cnt[i] = 0u;
    __syncthreads();
  }
  const long long first = (long long)blockIdx.x * (TR_THREADS * TR_CELL_PER_THREAD) + threadIdx.x;
  unsigned other = 0u;  // (the global table only) this thread's particles that count elsewhere
  for (int k0 = 0; k0 < TR_CELL_PER_THREAD; k0 += 8) {
    int64_t e[8];
    int32_t w[8];
    double px[8], py[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      const bool in = i < n;
      e[k] = in ? L.epoch[i] : -1;
      w[k] = in ? L.wall[i] : 0;
      px[k] = in ? L.x[i] : 0.0;
      py[k] = in ? L.y[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const long long i = first + (long long)(k0 + k) * TR_THREADS;
      int cell = (w[k] == wall && e[k] >= e_lo && e[k] <= e_hi) ? tr_cell(nx, ny, nz, bx, by, 1, px[k], py[k], 0.0) : cells;
      if (cell < 0 || cell > cells) cell = cells;  // (a landing place is never NaN)
      if (i >= n) cell = -1;
      if constexpr (LDS) tr_count_add(tr_cnt, cell);
      else if (cell == cells) ++other;
      else if (cell >= 0) atomicAdd(&total[cell], 1ull);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i <= cells; i += TR_THREADS) {
      const unsigned v = tr_cnt[i];
      if (v) atomicAdd(&total[i], (unsigned long long)v);
    }
  } else {  // "elsewhere" is ONE counter and may be most of the cloud: summed over the wavefront first, one atomic per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) other += __shfl_down(other, o);
    if ((threadIdx.x & 63) == 0 && other) atomicAdd(&total[cells], (unsigned long long)other);
  }
}

__device__ __forceinline__ double tr_wave_min(double v) { return -wave_max(-v); }

// partial[b * NM + q] of the workgroup's TR_CHUNK particles
__global__ void __launch_bounds__(TR_THREADS) k_tracers_partials(TrCloud c, int nx, int ny, double* __restrict__ partial) {
  __shared__ double lds[NM][TR_THREADS / 64];
  const long long first = (long long)blockIdx.x * TR_CHUNK + threadIdx.x;
  const double px = (double)nx, py = (double)ny;
  double s[NM];
#pragma unroll
  for (int q = 0; q < NM; ++q) s[q] = 0.0;
  s[10] = INFINITY;
  s[11] = -INFINITY;
#pragma unroll 4
  for (int k = 0; k < TR_PER_THREAD; ++k) {
    const long long i = first + (long long)k * TR_THREADS;
    if (i < c.n) {
      const double x = c.x[i], y = c.y[i], z = c.z[i];
      if (tr_lost(x, y, z)) {
        s[1] += 1.0;  // (the +0.0 a lost particle adds to the sums changes no bit of them)
      } else {
        const double x0 = c.x0[i], y0 = c.y0[i], z0 = c.z0[i];
        const double wx = (double)c.wx[i], wy = (double)c.wy[i];
        double t = x - x0;
        double w = wx * px;
        const double dx = t + w;
        t = y - y0;
        w = wy * py;
        const double dy = t + w;
        const double dz = z - z0;
        s[0] += 1.0;
        s[2] += dx;
        s[3] += dy;
        s[4] += dz;
        t = dx * dx;
        s[5] += t;
        t = dy * dy;
        s[6] += t;
        t = dz * dz;
        s[7] += t;
        s[8] += z;
        t = z * z;
        s[9] += t;
        s[10] = fmin(s[10], z);
        s[11] = fmax(s[11], z);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NM; ++q) {
    const double r = q < 10 ? wave_sum(s[q]) : q == 10 ? tr_wave_min(s[q]) : wave_max(s[q]);
    if (lane == 0) lds[q][wave] = r;
  }
  __syncthreads();
  if (threadIdx.x < NM) {
    const int q = threadIdx.x;
    double r = lds[q][0];
#pragma unroll
    for (int w = 1; w < TR_THREADS / 64; ++w) r = q < 10 ? r + lds[q][w] : q == 10 ? fmin(r, lds[q][w]) : fmax(r, lds[q][w]);
    partial[(long long)blockIdx.x * NM + q] = r;
  }
}

// out[q] = the partials in ascending workgroup order (sixteen loads in flight); no alive particle: z_min = z_max = 0
__global__ void __launch_bounds__(64) k_tracers_finish(const double* __restrict__ partial, int nwg, double* __restrict__ out) {
  __shared__ double sh[NM];
  const int q = threadIdx.x;
  if (q < NM) {
    const double* p = partial + q;
    double r = q < 10 ? 0.0 : q == 10 ? INFINITY : -INFINITY;
    for (int b0 = 0; b0 < nwg; b0 += 16) {
      double v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = b0 + k < nwg ? p[(long long)(b0 + k) * NM] : (q < 10 ? 0.0 : q == 10 ? INFINITY : -INFINITY);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (b0 + k < nwg) r = q < 10 ? r + v[k] : q == 10 ? fmin(r, v[k]) : fmax(r, v[k]);
    }
    sh[q] = r;
  }
  __syncthreads();
  if (q < NM) {
    double r = sh[q];
    if (q >= 10 && sh[0] == 0.0) r = 0.0;
    out[q] = r;
  }
}

// ---- the sort by cell --------------------------------------------------------------------------------------------------------

constexpr int TS_RUN = 4096;                    // items per workgroup of a pass: four waves of TS_ROUNDS rounds of 64
constexpr int TS_ROUNDS = TS_RUN / TR_THREADS;  // 16
constexpr int TS_SCAN = 4096;                   // table entries per workgroup of the scan: 256 threads of 16
constexpr uint32_t TR_KEY_LOST = 0xFFFFFFFFu;
typedef unsigned long long ts_item;             // key << 32 | slot

// the linear index of the first node an advance of this position loads (integer arithmetic only); lost: 0xFFFFFFFF
__host__ __device__ __forceinline__ uint32_t tr_sort_key(int nx, int ny, int nz, double x, double y, double z) {
  if (tr_lost(x, y, z)) return TR_KEY_LOST;
  const int i0 = tr_index(x, nx - 1), j0 = tr_index(y, ny - 1), k0 = tr_index(z, nz - 2);
  return (uint32_t)(((unsigned long long)k0 * (unsigned)ny + (unsigned)j0) * (unsigned)nx + (unsigned)i0);
}

__global__ void __launch_bounds__(TR_THREADS) k_tracers_sort_keys(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z, long long n,
                                                                  int nx, int ny, int nz, ts_item* __restrict__ items) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n) return;
  items[i] = ((ts_item)tr_sort_key(nx, ny, nz, x[i], y[i], z[i]) << 32) | (ts_item)i;
}

// hist[digit * nruns + run] = the run's items with that digit.  The tail of the last run (i >= n) is never loaded and counts
// nowhere (digit -1 in tr_count_add).
__global__ void __launch_bounds__(TR_THREADS) k_tracers_sort_hist(const ts_item* __restrict__ items, long long n, int shift, unsigned nruns, unsigned* __restrict__ hist) {
  __shared__ unsigned cnt[256];
  cnt[threadIdx.x] = 0u;
  const long long first = (long long)blockIdx.x * TS_RUN + threadIdx.x;
  ts_item v[TS_ROUNDS];
#pragma unroll
  for (int k = 0; k < TS_ROUNDS; ++k) {
    const long long i = first + (long long)k * TR_THREADS;
    v[k] = i < n ? items[i] : 0ull;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TS_ROUNDS; ++k) {
    const long long i = first + (long long)k * TR_THREADS;
    tr_count_add(cnt, i < n ? (int)((v[k] >> shift) & 255ull) : -1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nruns + blockIdx.x] = cnt[threadIdx.x];
}

// inclusive sum over the lanes of a wavefront
__device__ __forceinline__ unsigned ts_wave_scan(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// tab[e] becomes the sum of the entries before it INSIDE its chunk of TS_SCAN; sums[chunk] = the chunk's total.  `total` is a
// multiple of 256 (256 digits x nruns), so a thread's 16 consecutive entries lie inside the table or all outside it.
__global__ void __launch_bounds__(TR_THREADS) k_tracers_sort_scan(unsigned* __restrict__ tab, unsigned total, unsigned* __restrict__ sums) {
  __shared__ unsigned wsum[TR_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned base = blockIdx.x * (unsigned)TS_SCAN + threadIdx.x * 16u;
  const bool in = base < total;
  uint4 q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = in ? ((const uint4*)(tab + base))[k] : make_uint4(0u, 0u, 0u, 0u);
  unsigned s = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned t = q[k].x; q[k].x = s; s += t;
    t = q[k].y; q[k].y = s; s += t;
    t = q[k].z; q[k].z = s; s += t;
    t = q[k].w; q[k].w = s; s += t;
  }
  const unsigned inc = ts_wave_scan(s, lane);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  unsigned off = inc - s;
  for (int w = 0; w < wave; ++w) off += wsum[w];
  if (in) {
#pragma unroll
    for (int k = 0; k < 4; ++k) ((uint4*)(tab + base))[k] = make_uint4(q[k].x + off, q[k].y + off, q[k].z + off, q[k].w + off);
  }
  if (threadIdx.x == TR_THREADS - 1) sums[blockIdx.x] = off + s;
}

// sums[0 .. m) becomes its exclusive scan: one workgroup, 256 entries at a time with a carry
__global__ void __launch_bounds__(TR_THREADS) k_tracers_sort_scan_top(unsigned* __restrict__ sums, unsigned m) {
  __shared__ unsigned wsum[TR_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0u;
  for (unsigned b = 0; b < m; b += TR_THREADS) {
    const unsigned e = b + threadIdx.x;
    const unsigned v = e < m ? sums[e] : 0u;
    const unsigned inc = ts_wave_scan(v, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned off = carry + inc - v;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (e < m) sums[e] = off;
    carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// The stable scatter of one pass.  Wave w owns items [run*4096 + w*1024, + 1024) and the 256 counters cnt[w][]; after the count,
// cnt[w][d] is where the wave's first item of digit d goes: the scanned table entry of (d, run) plus the lower waves' counts.
// The wave then walks its 16 rounds in ascending order; the lanes of equal digit find each other with eight ballots, the rank of
// a lane is the counter plus the equal lanes below it, and the lowest of them moves the counter on.  Tail items of the last run
// (i >= n) are never loaded, take part in no ballot mask and write nothing; they are the highest lanes of the last rounds, so
// they change nobody's rank.  The ranks of a pass are a permutation of 0 .. n-1; the bound check keeps a broken table from
// writing outside the buffer.
__global__ void __launch_bounds__(TR_THREADS) k_tracers_sort_scatter(const ts_item* __restrict__ in, ts_item* __restrict__ out, long long n, int shift, unsigned nruns,
                                                                     const unsigned* __restrict__ hist, const unsigned* __restrict__ sums) {
  __shared__ unsigned cnt[TR_THREADS / 64][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < TR_THREADS / 64; ++w) cnt[w][threadIdx.x] = 0u;
  const long long first = (long long)blockIdx.x * TS_RUN + (long long)wave * (TS_ROUNDS * 64) + lane;
  ts_item v[TS_ROUNDS];
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const long long i = first + (long long)r * 64;
    v[r] = i < n ? in[i] : 0ull;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const long long i = first + (long long)r * 64;
    tr_count_add(cnt[wave], i < n ? (int)((v[r] >> shift) & 255ull) : -1);  // counts only: the order of these atomics decides nothing
  }
  __syncthreads();
  {
    const unsigned d = threadIdx.x;
    const unsigned e = d * nruns + blockIdx.x;
    unsigned g = hist[e] + sums[e / (unsigned)TS_SCAN];
#pragma unroll
    for (int w = 0; w < TR_THREADS / 64; ++w) {
      const unsigned t = cnt[w][d];
      cnt[w][d] = g;
      g += t;
    }
  }
  __syncthreads();
  volatile unsigned* mine = cnt[wave];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < TS_ROUNDS; ++r) {
    const long long i = first + (long long)r * 64;
    const bool valid = i < n;
    const unsigned d = (unsigned)((v[r] >> shift) & 255ull);
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bb = __ballot(valid && bit);
      m &= bit ? bb : ~bb;
    }
    // one lane per digit, the lowest, touches the counter and hands its value to the equal lanes above it
    const int lead = valid ? __ffsll((long long)m) - 1 : lane;
    unsigned at = 0u;
    if (valid && lane == lead) {
      at = mine[d];
      mine[d] = at + (unsigned)__popcll(m);
    }
    at = __shfl(at, lead);
    const unsigned rank = at + (unsigned)__popcll(m & below);
    if (valid && (long long)rank < n) out[rank] = v[r];
    __builtin_amdgcn_wave_barrier();  // the next round reads what this round's lowest lanes wrote (LDS serves a wave in order)
  }
}

// dst[s] = src[slot of items[s]]; src == nullptr: the slot itself (the ids of a cloud that was never sorted are 0 .. n-1).
// A slot is the low word of an item, formed from i < n in k_tracers_sort_keys and only moved since.
template <typename V>
__global__ void __launch_bounds__(TR_THREADS) k_tracers_sort_gather(const ts_item* __restrict__ items, const V* __restrict__ src, V* __restrict__ dst, long long n) {
  const long long s = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (s >= n) return;
  const unsigned slot = (unsigned)(items[s] & 0xFFFFFFFFull);
  if ((long long)slot >= n) return;
  dst[s] = src ? src[slot] : (V)slot;
}

// Host side of a context's cloud: made by the first ekpnp_tracers_seed / _set / _load / _arm, never by a context that uses none.
struct TracerState {
  long long n = 0;
  void* cloud = nullptr;      // one allocation: x, y, z, x0, y0, z0 [n] doubles, then wx, wy [n] int32, then the moments' partials and result
  size_t cloud_bytes = 0;
  int nwg = 0;                // workgroups of the moments: ceil(n / TR_CHUNK)
  double* part = nullptr;     // [nwg][NM], then out[NM] (inside `cloud`)
  unsigned long long* cells = nullptr;  // [EKPNP_TRACERS_MAX_CELLS + 1], made by the first ekpnp_tracers_cell_counts
  size_t cells_bytes = 0;
  double* tab = nullptr;      // GRID seeding: the three tables and their pinned host twin; `landed` marks the last upload
  double* tab_host = nullptr;
  size_t tab_doubles = 0;
  hipEvent_t landed = nullptr;
  Ring ring;                  // rows of NM doubles
  // the sort (both made by the first ekpnp_tracers_sort, dropped with the cloud they belong to): the two item buffers [n] each,
  // then the digit table [256][nruns] and its chunk sums; and ids [n], also made by a load of a file that carries ids
  void* sort = nullptr;
  size_t sort_bytes = 0;
  int32_t* ids = nullptr;
  size_t ids_bytes = 0;
  bool has_ids = false;       // false: the ids are 0 .. n-1, whatever `ids` holds
  int64_t epoch = 0;          // Brownian substeps taken since the cloud was seeded or set (a load restores it): the noise's clock
  double* samp = nullptr;     // ekpnp_tracers_sample's scratch [nvalues][n], grown on demand, dropped with the cloud
  size_t samp_bytes = 0;
  Ring tracks;                // rows of [ntags][5 + nvalues] doubles behind a header of four int32 tables [ntags] (TrTags)
  ekpnp_tracks_spec tspec{};  // the spec of the last ekpnp_tracks_arm and the size of the cloud it tagged (for the file)
  long long tracks_n = 0;
  // the landing record of the absorbing advance, made and cleared by the first ekpnp_tracers_advance_absorbing (or a load of its
  // file), dropped with the cloud it belongs to and by seed, set and load: 36 B per particle in the order of its file
  void* land = nullptr;
  size_t land_bytes = 0;
  TrLand land_dev() const {
    const size_t m = (size_t)n;
    int64_t* e = (int64_t*)land;
    double* d = (double*)(e + m);
    int32_t* w = (int32_t*)(d + 2 * m);
    return TrLand{e, d, d + m, w, w + m, w + 2 * m};
  }
  // the stretch record of the tangent advance, made by ekpnp_tracers_stretch_begin (or a load of its file), dropped like the landing
  // record: F [9][n] doubles, then e [n] int32, 76 B per particle, in slot order
  void* stretch = nullptr;
  size_t stretch_bytes = 0;
  TrStretch stretch_dev() const {
    double* F = (double*)stretch;
    return TrStretch{F, (int32_t*)(F + 9 * (size_t)n)};
  }
  TrCloud dev() const {
    double* d = (double*)cloud;
    const size_t m = (size_t)n;
    int32_t* w = (int32_t*)(d + 6 * m);
    return TrCloud{d, d + m, d + 2 * m, d + 3 * m, d + 4 * m, d + 5 * m, w, w + m, n};
  }
  double* out() const { return part + (size_t)nwg * NM; }
};

// the sort's scratch and the id array belong to a cloud of one size
static void tracers_sort_release(Ctx& c, TracerState& t) {
  if (t.sort) { (void)hipFree(t.sort); c.bytes -= t.sort_bytes; t.sort = nullptr; t.sort_bytes = 0; }
  if (t.ids) { (void)hipFree(t.ids); c.bytes -= t.ids_bytes; t.ids = nullptr; t.ids_bytes = 0; }
  t.has_ids = false;
  if (t.samp) { (void)hipFree(t.samp); c.bytes -= t.samp_bytes; t.samp = nullptr; t.samp_bytes = 0; }  // and so does the sample scratch
  if (t.land) { (void)hipFree(t.land); c.bytes -= t.land_bytes; t.land = nullptr; t.land_bytes = 0; }  // and the landing record
  if (t.stretch) { (void)hipFree(t.stretch); c.bytes -= t.stretch_bytes; t.stretch = nullptr; t.stretch_bytes = 0; }  // and the stretch record
}

// a new cloud has no landings (seed, set, load): the stream is waited for, an absorbing advance may still write the record
static int tracers_land_drop(Ctx& c, TracerState& t) {
  if (!t.land) return EKPNP_OK;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  (void)hipFree(t.land);
  c.bytes -= t.land_bytes;
  t.land = nullptr;
  t.land_bytes = 0;
  return EKPNP_OK;
}

// nor a stretch record (seed, set, load, ekpnp_tracers_stretch_end): the stream is waited for, a tangent advance may still write it
static int tracers_stretch_drop(Ctx& c, TracerState& t) {
  if (!t.stretch) return EKPNP_OK;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  (void)hipFree(t.stretch);
  c.bytes -= t.stretch_bytes;
  t.stretch = nullptr;
  t.stretch_bytes = 0;
  return EKPNP_OK;
}

void tracers_release(Ctx& c) {
  if (!c.tracers) return;
  TracerState& t = *c.tracers;
  tracers_sort_release(c, t);
  if (t.cloud) { (void)hipFree(t.cloud); c.bytes -= t.cloud_bytes; }
  if (t.cells) { (void)hipFree(t.cells); c.bytes -= t.cells_bytes; }
  if (t.tab) { (void)hipFree(t.tab); c.bytes -= t.tab_doubles * sizeof(double); }
  if (t.tab_host) (void)hipHostFree(t.tab_host);
  if (t.landed) (void)hipEventDestroy(t.landed);
  if (t.ring.alloc) c.bytes -= t.ring.bytes;
  ring_release(t.ring);
  if (t.tracks.alloc) c.bytes -= t.tracks.bytes;
  ring_release(t.tracks);
  delete c.tracers;
  c.tracers = nullptr;
}

static std::string num(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.17g", v);
  return b;
}

static int tracers_check_lattice(const ekpnp_params& p, std::string& err) {
  if (p.nx < 1 || p.ny < 1) { err = "tracers: nx = " + std::to_string(p.nx) + ", ny = " + std::to_string(p.ny) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (p.nz < 3) { err = "tracers: nz = " + std::to_string(p.nz) + " (must be >= 3: there is no interior plane)"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

static int tracers_check_spec(const ekpnp_params& p, const ekpnp_tracers_spec* s, std::string& err) {
  if (!s) { err = "tracers: NULL spec"; return EKPNP_ERR_INVALID; }
  if (int rc = tracers_check_lattice(p, err)) return rc;
  if (s->n < 1 || s->n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)s->n) + " outside 1 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); return EKPNP_ERR_INVALID; }
  if (s->mode < 0 || s->mode > 1) { err = "tracers: mode = " + std::to_string(s->mode) + " (must be 0 or 1)"; return EKPNP_ERR_INVALID; }
  const int g[3] = {s->gx, s->gy, s->gz};
  const char* const gn[3] = {"gx", "gy", "gz"};
  if (s->mode == EKPNP_TRACERS_GRID) {
    for (int a = 0; a < 3; ++a)
      if (g[a] < 1) { err = std::string("tracers: ") + gn[a] + " = " + std::to_string(g[a]) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
    const __int128 prod = (__int128)s->gx * s->gy * s->gz;
    if (prod != (__int128)s->n) {
      err = "tracers: gx*gy*gz = " + std::to_string(s->gx) + "*" + std::to_string(s->gy) + "*" + std::to_string(s->gz) + " is not n = " + std::to_string((long long)s->n);
      return EKPNP_ERR_INVALID;
    }
  } else {
    for (int a = 0; a < 3; ++a)
      if (g[a] != 0) { err = std::string("tracers: ") + gn[a] + " = " + std::to_string(g[a]) + " (must be 0 for random seeding)"; return EKPNP_ERR_INVALID; }
  }
  const double top[3] = {(double)p.nx, (double)p.ny, (double)(p.nz - 1)};
  const char* const an[3] = {"x", "y", "z"};
  for (int a = 0; a < 3; ++a) {
    const std::string w = std::string("tracers: box ") + an[a] + ": ";
    if (!std::isfinite(s->lo[a])) { err = w + "lo = " + num(s->lo[a]) + " (must be finite)"; return EKPNP_ERR_INVALID; }
    if (!std::isfinite(s->hi[a])) { err = w + "hi = " + num(s->hi[a]) + " (must be finite)"; return EKPNP_ERR_INVALID; }
    if (!(s->hi[a] > s->lo[a])) { err = w + "hi = " + num(s->hi[a]) + " is not above lo = " + num(s->lo[a]); return EKPNP_ERR_INVALID; }
    if (s->lo[a] < 0.0) { err = w + "lo = " + num(s->lo[a]) + " below 0"; return EKPNP_ERR_INVALID; }
    if (s->hi[a] > top[a]) { err = w + "hi = " + num(s->hi[a]) + " above " + num(top[a]); return EKPNP_ERR_INVALID; }
  }
  return EKPNP_OK;
}

static inline double tr_period(const ekpnp_params& p, int axis) { return axis == 0 ? (double)p.nx : axis == 1 ? (double)p.ny : INFINITY; }

// GRID: coordinate i of g along an axis (host arithmetic, the device indexes the table)
static double tr_grid_value(int i, int g, double lo, double hi, double period) {
  const double w = hi - lo;
  const double c = (double)i + 0.5;
  const double m = c * w;
  const double q = m / (double)g;
  const double v = lo + q;
  return (v >= hi || v >= period) ? lo : v;
}

// all three NaN, or inside the invariant
static bool tr_position_ok(const ekpnp_params& p, double x, double y, double z) {
  if (x != x && y != y && z != z) return true;
  return x >= 0.0 && x < (double)p.nx && y >= 0.0 && y < (double)p.ny && z >= 0.0 && z <= (double)(p.nz - 1);
}

static int tracers_check_cells(const ekpnp_params& p, int bx, int by, int bz, std::string& err) {
  if (int rc = tracers_check_lattice(p, err)) return rc;
  if (bx < 1 || bx > p.nx) { err = "tracers: bx = " + std::to_string(bx) + " outside 1 .. " + std::to_string(p.nx); return EKPNP_ERR_INVALID; }
  if (by < 1 || by > p.ny) { err = "tracers: by = " + std::to_string(by) + " outside 1 .. " + std::to_string(p.ny); return EKPNP_ERR_INVALID; }
  if (bz < 1 || bz > p.nz - 1) { err = "tracers: bz = " + std::to_string(bz) + " outside 1 .. " + std::to_string(p.nz - 1); return EKPNP_ERR_INVALID; }
  const long long cells = (long long)bx * by * bz;
  if (cells > EKPNP_TRACERS_MAX_CELLS) { err = "tracers: bx*by*bz = " + std::to_string(cells) + " above " + std::to_string(EKPNP_TRACERS_MAX_CELLS); return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

static int tracers_check_advance(double mu, double h, int nsub, std::string& err) {
  if (!std::isfinite(mu)) { err = "tracers: mu = " + num(mu) + " (must be finite)"; return EKPNP_ERR_INVALID; }
  if (!std::isfinite(h)) { err = "tracers: h = " + num(h) + " (must be finite)"; return EKPNP_ERR_INVALID; }
  if (nsub < 1 || nsub > 4096) { err = "tracers: nsub = " + std::to_string(nsub) + " outside 1 .. 4096"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

// the diffusivity of a Brownian advance beside tracers_check_advance: D finite and >= 0, and 6 D h >= 0 and finite (its root is taken)
static int tracers_check_brownian(double D, double h, std::string& err) {
  if (!std::isfinite(D) || D < 0.0) { err = "tracers: D = " + num(D) + " (must be finite and >= 0)"; return EKPNP_ERR_INVALID; }
  const double t = 6.0 * D;
  const double m = t * h;
  if (!(m >= 0.0) || !std::isfinite(m)) { err = "tracers: D*h = " + num(D * h) + " (must be >= 0, and 6*D*h finite: diffusion does not run backwards)"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

static const char* const kValueNames[TR_MAXV] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T", "q"};

// the values of a sample (min_values 1) or of a track (0: positions only)
static int tracers_check_values(const ekpnp_params& p, int nvalues, const int32_t* values, int min_values, std::string& err) {
  if (int rc = tracers_check_lattice(p, err)) return rc;
  if (nvalues < min_values || nvalues > TR_MAXV) { err = "tracers: nvalues = " + std::to_string(nvalues) + " outside " + std::to_string(min_values) + " .. " + std::to_string(TR_MAXV); return EKPNP_ERR_INVALID; }
  if (nvalues > 0 && !values) { err = "tracers: NULL values"; return EKPNP_ERR_INVALID; }
  for (int v = 0; v < nvalues; ++v) {
    if (values[v] < 0 || values[v] > EKPNP_TRACERS_Q) { err = "tracers: value id " + std::to_string(values[v]) + " (place " + std::to_string(v) + ") outside 0 .. " + std::to_string(EKPNP_TRACERS_Q); return EKPNP_ERR_INVALID; }
    for (int w = 0; w < v; ++w)
      if (values[w] == values[v]) { err = "tracers: value id " + std::to_string(values[v]) + " is named twice (places " + std::to_string(w) + " and " + std::to_string(v) + ")"; return EKPNP_ERR_INVALID; }
  }
  return EKPNP_OK;
}

static int tracers_check_tracks(const ekpnp_params& p, int64_t n, const ekpnp_tracks_spec* s, std::string& err) {
  if (!s) { err = "tracers: NULL spec"; return EKPNP_ERR_INVALID; }
  if (int rc = tracers_check_values(p, s->nvalues, s->values, 0, err)) return rc;
  if (n < 1 || n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)n) + " outside 1 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); return EKPNP_ERR_INVALID; }
  if (s->ntags < 1 || s->ntags > EKPNP_TRACERS_MAX_TRACKS) { err = "tracers: ntags = " + std::to_string(s->ntags) + " outside 1 .. " + std::to_string(EKPNP_TRACERS_MAX_TRACKS); return EKPNP_ERR_INVALID; }
  std::vector<int32_t> seen(s->ids, s->ids + s->ntags);
  for (int k = 0; k < s->ntags; ++k)
    if (s->ids[k] < 0 || (int64_t)s->ids[k] >= n) { err = "tracers: tag " + std::to_string(k) + " is id " + std::to_string(s->ids[k]) + ", outside 0 .. " + std::to_string((long long)n - 1); return EKPNP_ERR_INVALID; }
  std::sort(seen.begin(), seen.end());
  for (int k = 1; k < s->ntags; ++k)
    if (seen[(size_t)k] == seen[(size_t)k - 1]) { err = "tracers: id " + std::to_string(seen[(size_t)k]) + " is tagged twice"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

// the groups of a checked list of values over the arrays fld[EKPNP_NFIELDS]: in slot order, a group is closed when the next
// value's arrays (q: two) would make more than TR_GROUP
static TrSample tr_sample_plan(const ekpnp_params& p, int nvalues, const int32_t* values, const double* const* fld) {
  TrSample a{};
  a.nvalues = nvalues;
  a.nx = p.nx;
  a.ny = p.ny;
  a.nz = p.nz;
  for (int v = 0; v < nvalues; ++v) {
    const bool q = values[v] == EKPNP_TRACERS_Q;
    const int cost = q ? 2 : 1;
    if (a.ngroups == 0 || a.g[a.ngroups - 1].narr + cost > TR_GROUP) ++a.ngroups;
    TrGroup& G = a.g[a.ngroups - 1];
    const int e = G.narr;
    G.op[e] = q ? TR_OP_Q : TR_OP_VALUE;
    G.slot[e] = (int8_t)v;
    G.p[e] = fld[q ? EKPNP_C : values[v]];
    if (q) G.p[e + 1] = fld[EKPNP_CN];
    G.narr = (int16_t)(e + cost);
  }
  return a;
}

static inline bool tr_names_phi_or_e(int nvalues, const int32_t* values) {
  for (int v = 0; v < nvalues; ++v)
    if (values[v] == EKPNP_PHI || values[v] == EKPNP_EX || values[v] == EKPNP_EY || values[v] == EKPNP_EZ) return true;
  return false;
}

static TrStep tr_step_of(const ekpnp_params& p, double mu, double h, int nsub) {
  TrStep s{};
  s.hx = h / p.dx;
  s.hy = h / p.dy;
  s.hz = h / p.dz;
  s.ax = 0.5 * s.hx;
  s.ay = 0.5 * s.hy;
  s.az = 0.5 * s.hz;
  s.mu = mu;
  s.nx = p.nx;
  s.ny = p.ny;
  s.nz = p.nz;
  s.nsub = nsub;
  return s;
}

// the kick lengths sqrt(6 D h) in cells, operation by operation: the host's square root is correctly rounded
static TrNoise tr_noise_of(const ekpnp_params& p, double D, double h, uint64_t seed, int64_t epoch) {
  TrNoise q{};
  const double t = 6.0 * D;
  const double m = t * h;
  const double r = std::sqrt(m);
  q.kx = r / p.dx;
  q.ky = r / p.dy;
  q.kz = r / p.dz;
  q.seed = seed;
  q.epoch = epoch;
  return q;
}

}  // namespace ekpnp

// ---- host only ---------------------------------------------------------------------------------------------------------------

extern "C" int ekpnp_tracers_spec_check(const ekpnp_params* p, const ekpnp_tracers_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else rc = tracers_check_spec(*p, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_tracers_seed_host(const ekpnp_params* p, const ekpnp_tracers_spec* spec, int64_t first, int64_t count, double* x, double* y, double* z) {
  if (int rc = ekpnp_tracers_spec_check(p, spec)) return rc;
  if (first < 0 || count < 0 || first > spec->n || count > spec->n - first) {
    set_create_error("tracers: particles " + std::to_string((long long)first) + " .. " + std::to_string((long long)(first + count - 1)) + " are not inside n = " + std::to_string((long long)spec->n));
    return EKPNP_ERR_INVALID;
  }
  if (count == 0) return EKPNP_OK;
  if (!x || !y || !z) { set_create_error("tracers: NULL pointer"); return EKPNP_ERR_INVALID; }
  double* const out[3] = {x, y, z};
  if (spec->mode == EKPNP_TRACERS_GRID) {
    const int g[3] = {spec->gx, spec->gy, spec->gz};
    for (int64_t q = 0; q < count; ++q) {
      const int64_t pi = first + q, row = pi / g[0];
      const int idx[3] = {(int)(pi - row * g[0]), (int)(row % g[1]), (int)(row / g[1])};
      for (int a = 0; a < 3; ++a) out[a][q] = tr_grid_value(idx[a], g[a], spec->lo[a], spec->hi[a], tr_period(*p, a));
    }
  } else {
    for (int a = 0; a < 3; ++a) {
      const double t = spec->hi[a] - spec->lo[a];
      for (int64_t q = 0; q < count; ++q) out[a][q] = tr_seed_random(spec->seed, (uint64_t)(first + q), a, spec->lo[a], spec->hi[a], t, tr_period(*p, a));
    }
  }
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_advance_host(const ekpnp_params* p, const double* ux, const double* uy, const double* uz, const double* ex, const double* ey,
                                          const double* ez, double mu, double h, int nsub, int64_t n, double* x, double* y, double* z, int32_t* wx, int32_t* wy) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else if ((rc = tracers_check_lattice(*p, err)) == EKPNP_OK && (rc = tracers_check_advance(mu, h, nsub, err)) == EKPNP_OK) {
    if (n < 0 || n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)n) + " outside 0 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); rc = EKPNP_ERR_INVALID; }
    else if (!ux || !uy || !uz || !x || !y || !z || !wx || !wy || (mu != 0.0 && (!ex || !ey || !ez))) { err = "tracers: NULL pointer"; rc = EKPNP_ERR_INVALID; }
  }
  if (rc) { set_create_error(err); return rc; }
  const TrFields f{{ux, uy, uz}, {ex, ey, ez}};
  const TrStep s = tr_step_of(*p, mu, h, nsub);
  for (int64_t i = 0; i < n; ++i) {
    if (tr_lost(x[i], y[i], z[i])) continue;
    int a = wx[i], b = wy[i];
    if (mu != 0.0) tr_advance<true>(f, s, x[i], y[i], z[i], a, b);
    else tr_advance<false>(f, s, x[i], y[i], z[i], a, b);
    wx[i] = a;
    wy[i] = b;
  }
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_advance_tangent_host(const ekpnp_params* p, const double* ux, const double* uy, const double* uz, const double* ex, const double* ey,
                                                  const double* ez, double mu, double h, int nsub, int64_t n, double* x, double* y, double* z, int32_t* wx, int32_t* wy,
                                                  double* F, int32_t* e) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else if ((rc = tracers_check_lattice(*p, err)) == EKPNP_OK && (rc = tracers_check_advance(mu, h, nsub, err)) == EKPNP_OK) {
    if (n < 0 || n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)n) + " outside 0 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); rc = EKPNP_ERR_INVALID; }
    else if (!ux || !uy || !uz || !x || !y || !z || !wx || !wy || !F || !e || (mu != 0.0 && (!ex || !ey || !ez))) { err = "tracers: NULL pointer"; rc = EKPNP_ERR_INVALID; }
  }
  if (rc) { set_create_error(err); return rc; }
  const TrFields f{{ux, uy, uz}, {ex, ey, ez}};
  const TrStep s = tr_step_of(*p, mu, h, nsub);
  for (int64_t i = 0; i < n; ++i) {
    if (tr_lost(x[i], y[i], z[i])) continue;
    int a = wx[i], b = wy[i], lev = e[i];
    double Fi[9];
    for (int q = 0; q < 9; ++q) Fi[q] = F[(size_t)q * (size_t)n + (size_t)i];
    if (mu != 0.0) tr_advance_tangent<true>(f, s, x[i], y[i], z[i], a, b, Fi, lev);
    else tr_advance_tangent<false>(f, s, x[i], y[i], z[i], a, b, Fi, lev);
    wx[i] = a;
    wy[i] = b;
    for (int q = 0; q < 9; ++q) F[(size_t)q * (size_t)n + (size_t)i] = Fi[q];
    e[i] = lev;
  }
  return EKPNP_OK;
}

extern "C" int32_t ekpnp_stretch_level(const double F[9], int32_t e) {
  return F ? tr_stretch_level(F, e) : TR_NO_LEVEL;
}

extern "C" void ekpnp_tracers_kick(uint64_t seed, int64_t id, int64_t epoch, double r[3]) {
  if (r) tr_kick(seed, id, epoch, r);
}

extern "C" int ekpnp_tracers_advance_brownian_host(const ekpnp_params* p, const double* ux, const double* uy, const double* uz, const double* ex, const double* ey,
                                                   const double* ez, int64_t n, const int32_t* ids, double* x, double* y, double* z, int32_t* wx, int32_t* wy,
                                                   double mu, double D, double h, int nsub, uint64_t seed, int64_t epoch) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else if ((rc = tracers_check_lattice(*p, err)) == EKPNP_OK && (rc = tracers_check_advance(mu, h, nsub, err)) == EKPNP_OK && (rc = tracers_check_brownian(D, h, err)) == EKPNP_OK) {
    if (n < 0 || n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)n) + " outside 0 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); rc = EKPNP_ERR_INVALID; }
    else if (epoch < 0 || epoch > INT64_MAX - nsub) { err = "tracers: epoch = " + std::to_string((long long)epoch) + " (must be >= 0, and epoch + nsub must fit 63 bits)"; rc = EKPNP_ERR_INVALID; }
    else if (!ux || !uy || !uz || !x || !y || !z || !wx || !wy || (mu != 0.0 && (!ex || !ey || !ez))) { err = "tracers: NULL pointer"; rc = EKPNP_ERR_INVALID; }
  }
  if (rc) { set_create_error(err); return rc; }
  const TrFields f{{ux, uy, uz}, {ex, ey, ez}};
  const TrStep s = tr_step_of(*p, mu, h, nsub);
  const TrNoise q = tr_noise_of(*p, D, h, seed, epoch);
  for (int64_t i = 0; i < n; ++i) {
    if (tr_lost(x[i], y[i], z[i])) continue;
    const int64_t id = ids ? (int64_t)ids[i] : i;
    int a = wx[i], b = wy[i];
    if (mu != 0.0) tr_advance_brownian<true>(f, s, q, id, x[i], y[i], z[i], a, b);
    else tr_advance_brownian<false>(f, s, q, id, x[i], y[i], z[i], a, b);
    wx[i] = a;
    wy[i] = b;
  }
  return EKPNP_OK;
}

static int tracers_check_walls(int walls, std::string& err) {
  if (walls < 1 || walls > 3) { err = "tracers: walls = " + std::to_string(walls) + " outside 1 .. 3 (1: the bottom plate absorbs, 2: the top plate, 3: both)"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_advance_absorbing_host(const ekpnp_params* p, const double* ux, const double* uy, const double* uz, const double* ex, const double* ey,
                                                    const double* ez, int64_t n, const int32_t* ids, double* x, double* y, double* z, int32_t* wx, int32_t* wy,
                                                    double mu, double D, double h, int nsub, uint64_t seed, int64_t epoch, int walls, int64_t* land_epoch,
                                                    int32_t* land_wall, double* land_x, double* land_y, int32_t* land_wx, int32_t* land_wy) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else if ((rc = tracers_check_lattice(*p, err)) == EKPNP_OK && (rc = tracers_check_advance(mu, h, nsub, err)) == EKPNP_OK && (rc = tracers_check_brownian(D, h, err)) == EKPNP_OK &&
           (rc = tracers_check_walls(walls, err)) == EKPNP_OK) {
    if (n < 0 || n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)n) + " outside 0 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); rc = EKPNP_ERR_INVALID; }
    else if (epoch < 0 || epoch > INT64_MAX - nsub) { err = "tracers: epoch = " + std::to_string((long long)epoch) + " (must be >= 0, and epoch + nsub must fit 63 bits)"; rc = EKPNP_ERR_INVALID; }
    else if (!ux || !uy || !uz || !x || !y || !z || !wx || !wy || (mu != 0.0 && (!ex || !ey || !ez)) || !land_epoch || !land_wall || !land_x || !land_y || !land_wx || !land_wy) {
      err = "tracers: NULL pointer";
      rc = EKPNP_ERR_INVALID;
    }
    for (int64_t i = 0; i < n && rc == EKPNP_OK; ++i) {
      if (ids && (ids[i] < 0 || (int64_t)ids[i] >= n)) { err = "tracers: slot " + std::to_string((long long)i) + " holds id " + std::to_string(ids[i]) + ", outside 0 .. " + std::to_string((long long)n - 1); rc = EKPNP_ERR_INVALID; }
      else if (land_wall[i] < 0 || land_wall[i] > 2) { err = "tracers: landing record of id " + std::to_string((long long)i) + ": wall = " + std::to_string(land_wall[i]) + " outside 0 .. 2"; rc = EKPNP_ERR_INVALID; }
      else if (land_epoch[i] < 0 && land_wall[i] != 0) { err = "tracers: landing record of id " + std::to_string((long long)i) + ": epoch = " + std::to_string((long long)land_epoch[i]) + " with wall = " + std::to_string(land_wall[i]) + " (no landing has wall 0)"; rc = EKPNP_ERR_INVALID; }
    }
  }
  if (rc) { set_create_error(err); return rc; }
  const TrFields f{{ux, uy, uz}, {ex, ey, ez}};
  const TrStep s = tr_step_of(*p, mu, h, nsub);
  const TrNoise q = tr_noise_of(*p, D, h, seed, epoch);
  const double top = (double)(p->nz - 1);
  for (int64_t i = 0; i < n; ++i) {
    if (tr_lost(x[i], y[i], z[i])) continue;
    const int64_t id = ids ? (int64_t)ids[i] : i;
    int wall = tr_on_plate(walls, z[i], top);
    int64_t when = epoch;
    int a = wx[i], b = wy[i];
    if (!wall) {  // (a stuck particle: no substep, no draw, no store to the cloud)
      int at = 0;
      if (mu != 0.0) wall = tr_advance_absorbing<true>(f, s, q, walls, id, x[i], y[i], z[i], a, b, at);
      else wall = tr_advance_absorbing<false>(f, s, q, walls, id, x[i], y[i], z[i], a, b, at);
      wx[i] = a;
      wy[i] = b;
      when = epoch + (int64_t)at + 1;
    }
    if (wall && land_epoch[id] < 0) {  // a FIRST-passage record
      land_epoch[id] = when;
      land_wall[id] = wall;
      land_x[id] = x[i];
      land_y[id] = y[i];
      land_wx[id] = a;
      land_wy[id] = b;
    }
  }
  return EKPNP_OK;
}

static int landings_check_hist(int walls, int64_t e0, int64_t width, int nbins, std::string& err) {
  if (int rc = tracers_check_walls(walls, err)) return rc;
  if (e0 < 0) { err = "tracers: e0 = " + std::to_string((long long)e0) + " (must be >= 0)"; return EKPNP_ERR_INVALID; }
  if (width < 1) { err = "tracers: width = " + std::to_string((long long)width) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (nbins < 1 || nbins > 4096) { err = "tracers: nbins = " + std::to_string(nbins) + " outside 1 .. 4096"; return EKPNP_ERR_INVALID; }
  return EKPNP_OK;
}

extern "C" int ekpnp_landings_bin(int64_t e0, int64_t width, int nbins, int64_t epoch) {
  std::string err;
  if (landings_check_hist(3, e0, width, nbins, err)) { set_create_error(err); return -1; }
  return tr_land_bin(e0, width, nbins, epoch);
}

extern "C" int ekpnp_tracers_cell(const ekpnp_params* p, int bx, int by, int bz, double x, double y, double z) {
  std::string err;
  if (!p) { set_create_error("tracers: NULL parameters"); return -2; }
  if (tracers_check_cells(*p, bx, by, bz, err)) { set_create_error(err); return -2; }
  return tr_cell(p->nx, p->ny, p->nz, bx, by, bz, x, y, z);
}

// keys are 32-bit and 0xFFFFFFFF is the lost particles': the largest key nx*ny*(nz-1) - 1 must stay below it
static int tracers_check_sort_lattice(const ekpnp_params& p, std::string& err) {
  if (int rc = tracers_check_lattice(p, err)) return rc;
  const unsigned __int128 prod = (unsigned __int128)(unsigned)p.nx * (unsigned)p.ny * (unsigned)(p.nz - 1);
  if (prod >= (unsigned __int128)0xFFFFFFFFull) {
    err = "tracers: nx*ny*(nz-1) = " + std::to_string((unsigned long long)prod) + " does not fit a 32-bit sort key (must be below 4294967295)";
    return EKPNP_ERR_INVALID;
  }
  return EKPNP_OK;
}

extern "C" uint32_t ekpnp_tracers_sort_key(const ekpnp_params* p, double x, double y, double z) {
  std::string err;
  if (!p) { set_create_error("tracers: NULL parameters"); return TR_KEY_LOST; }
  if (tracers_check_sort_lattice(*p, err)) { set_create_error(err); return TR_KEY_LOST; }
  return tr_sort_key(p->nx, p->ny, p->nz, x, y, z);
}

extern "C" int ekpnp_tracers_sort_host(const ekpnp_params* p, int64_t n, const double* x, const double* y, const double* z, int32_t* perm) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else if ((rc = tracers_check_sort_lattice(*p, err)) == EKPNP_OK) {
    if (n < 0 || n > EKPNP_TRACERS_MAX_N) { err = "tracers: n = " + std::to_string((long long)n) + " outside 0 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); rc = EKPNP_ERR_INVALID; }
    else if (n > 0 && (!x || !y || !z || !perm)) { err = "tracers: NULL pointer"; rc = EKPNP_ERR_INVALID; }
  }
  if (rc) { set_create_error(err); return rc; }
  // key << 32 | slot: every item is different, so the ascending order of the items IS the stable order of the keys
  std::vector<ts_item> items((size_t)n);
  for (int64_t i = 0; i < n; ++i) items[(size_t)i] = ((ts_item)tr_sort_key(p->nx, p->ny, p->nz, x[i], y[i], z[i]) << 32) | (ts_item)i;
  std::sort(items.begin(), items.end());
  for (int64_t s = 0; s < n; ++s) perm[s] = (int32_t)(items[(size_t)s] & 0xFFFFFFFFull);
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_values_check(const ekpnp_params* p, int nvalues, const int32_t* values) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else rc = tracers_check_values(*p, nvalues, values, 1, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_tracks_spec_check(const ekpnp_params* p, int64_t n, const ekpnp_tracks_spec* spec) {
  std::string err;
  int rc = EKPNP_ERR_INVALID;
  if (!p) err = "tracers: NULL parameters";
  else rc = tracers_check_tracks(*p, n, spec, err);
  if (rc) set_create_error(err);
  return rc;
}

extern "C" int ekpnp_tracers_sample_host(const ekpnp_params* p, int nvalues, const int32_t* values, const double* const* fields, int64_t n, const double* x,
                                         const double* y, const double* z, double* out) {
  if (int rc = ekpnp_tracers_values_check(p, nvalues, values)) return rc;
  std::string err;
  if (n < 0 || n > EKPNP_TRACERS_MAX_N) err = "tracers: n = " + std::to_string((long long)n) + " outside 0 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N);
  else if (!fields || (n > 0 && (!x || !y || !z || !out))) err = "tracers: NULL pointer";
  else
    for (int v = 0; v < nvalues && err.empty(); ++v) {
      const bool q = values[v] == EKPNP_TRACERS_Q;
      if (!fields[q ? EKPNP_C : values[v]] || (q && !fields[EKPNP_CN])) err = std::string("tracers: value ") + kValueNames[values[v]] + " is named and its array is NULL";
    }
  if (!err.empty()) { set_create_error(err); return EKPNP_ERR_INVALID; }
  const TrSample a = tr_sample_plan(*p, nvalues, values, fields);
  for (int64_t i = 0; i < n; ++i) tr_sample(a, x[i], y[i], z[i], out + i, (long long)n);
  return EKPNP_OK;
}

// ---- the cloud ---------------------------------------------------------------------------------------------------------------

#define NEEDSINGLE(ctx) \
  NEEDCTX(ctx);         \
  if (c.slab) return fail(c, kSlabMsg)

static int need_tracers(Ctx& c) {
  if (c.tracers) return EKPNP_OK;
  if (int rc = tracers_check_lattice(c.p, c.err)) return rc;
  c.tracers = new (std::nothrow) TracerState();
  if (!c.tracers) { c.err = "host allocation failed"; return EKPNP_ERR_NOMEM; }
  return EKPNP_OK;
}

// a cloud of n particles (the old allocation if n is unchanged; otherwise the stream is waited for: a pass may still read it)
static int tracers_alloc(Ctx& c, long long n) {
  if (int rc = need_tracers(c)) return rc;
  TracerState& t = *c.tracers;
  if (t.cloud && t.n == n) return EKPNP_OK;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  if (t.cloud) { (void)hipFree(t.cloud); c.bytes -= t.cloud_bytes; t.cloud = nullptr; t.cloud_bytes = 0; t.n = 0; t.part = nullptr; }
  tracers_sort_release(c, t);
  const int nwg = (int)((n + TR_CHUNK - 1) / TR_CHUNK);
  const size_t bytes = (size_t)n * 56 + ((size_t)nwg + 1) * NM * sizeof(double);  // (56 n is a multiple of 8: the partials are aligned)
  HIPCHK(c, hipMalloc(&t.cloud, bytes));
  t.cloud_bytes = bytes;
  c.bytes += bytes;
  t.n = n;
  t.nwg = nwg;
  t.part = (double*)((char*)t.cloud + (size_t)n * 56);
  return EKPNP_OK;
}

static inline TracerState* cloud_of(Ctx& c) { return c.tracers && c.tracers->cloud ? c.tracers : nullptr; }
static inline unsigned tr_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// upload a whole cloud from host arrays (synchronous)
static int tracers_upload(Ctx& c, long long n, const double* const pos[6], const int32_t* wx, const int32_t* wy) {
  if (int rc = tracers_alloc(c, n)) return rc;
  if (int rc = tracers_land_drop(c, *c.tracers)) return rc;
  if (int rc = tracers_stretch_drop(c, *c.tracers)) return rc;
  c.tracers->has_ids = false;  // a new cloud: slot s holds particle s (a load that carries ids puts them back)
  c.tracers->epoch = 0;        // and no Brownian substep was taken (a load puts its file's epoch back)
  c.tracers->tracks.armed = false;  // and the tags of an armed track ring named particles of the old one
  const TrCloud d = c.tracers->dev();
  double* const dst[6] = {d.x, d.y, d.z, d.x0, d.y0, d.z0};
  for (int a = 0; a < 6; ++a) HIPCHK(c, hipMemcpyAsync(dst[a], pos[a], (size_t)n * sizeof(double), hipMemcpyHostToDevice, c.stream));
  if (wx) {
    HIPCHK(c, hipMemcpyAsync(d.wx, wx, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
    HIPCHK(c, hipMemcpyAsync(d.wy, wy, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
  } else {
    HIPCHK(c, hipMemsetAsync(d.wx, 0, 2 * (size_t)n * sizeof(int32_t), c.stream));
  }
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_seed(ekpnp_ctx* ctx, const ekpnp_tracers_spec* spec) {
  NEEDSINGLE(ctx);
  if (int rc = tracers_check_spec(c.p, spec, c.err)) return rc;
  if (int rc = tracers_alloc(c, (long long)spec->n)) return rc;
  TracerState& t = *c.tracers;
  if (int rc = tracers_land_drop(c, t)) return rc;
  if (int rc = tracers_stretch_drop(c, t)) return rc;
  t.has_ids = false;
  t.epoch = 0;
  t.tracks.armed = false;  // the tags named particles of the cloud that is replaced here (the rows stay readable)
  TrSeedArgs a{};
  for (int q = 0; q < 3; ++q) {
    a.lo[q] = spec->lo[q];
    a.hi[q] = spec->hi[q];
    a.t[q] = spec->hi[q] - spec->lo[q];
    a.period[q] = tr_period(c.p, q);
  }
  a.seed = spec->seed;
  a.mode = spec->mode;
  a.gx = spec->gx;
  a.gy = spec->gy;
  a.gz = spec->gz;
  if (spec->mode == EKPNP_TRACERS_GRID) {
    const size_t need = (size_t)spec->gx + (size_t)spec->gy + (size_t)spec->gz;
    if (need > t.tab_doubles) {
      HIPCHK(c, hipStreamSynchronize(c.stream));  // an earlier seed may still read the old tables
      if (t.tab) { (void)hipFree(t.tab); c.bytes -= t.tab_doubles * sizeof(double); t.tab = nullptr; }
      if (t.tab_host) { (void)hipHostFree(t.tab_host); t.tab_host = nullptr; }
      t.tab_doubles = 0;
      HIPCHK(c, hipMalloc((void**)&t.tab, need * sizeof(double)));
      t.tab_doubles = need;
      c.bytes += need * sizeof(double);
      HIPCHK(c, hipHostMalloc((void**)&t.tab_host, need * sizeof(double), hipHostMallocDefault));
      if (!t.landed) HIPCHK(c, hipEventCreateWithFlags(&t.landed, hipEventDisableTiming));
    } else {
      if (!t.tab || !t.tab_host || !t.landed) { c.err = "tracers: the table buffer could not be made earlier"; return EKPNP_ERR_HIP; }
      HIPCHK(c, hipEventSynchronize(t.landed));  // the previous upload has left the pinned twin (not a wait for the stream)
    }
    const int g[3] = {spec->gx, spec->gy, spec->gz};
    double* h = t.tab_host;
    for (int q = 0; q < 3; ++q)
      for (int i = 0; i < g[q]; ++i) *h++ = tr_grid_value(i, g[q], spec->lo[q], spec->hi[q], a.period[q]);
    HIPCHK(c, hipMemcpyAsync(t.tab, t.tab_host, need * sizeof(double), hipMemcpyHostToDevice, c.stream));
    HIPCHK(c, hipEventRecord(t.landed, c.stream));
    a.tab = t.tab;
  }
  hipLaunchKernelGGL(k_tracers_seed, dim3(tr_blocks(t.n, TR_THREADS)), dim3(TR_THREADS), 0, c.stream, a, t.dev());
  note_launch(c, "k_tracers_seed");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_set(ekpnp_ctx* ctx, int64_t n, const double* x, const double* y, const double* z) {
  NEEDSINGLE(ctx);
  if (n < 1 || n > EKPNP_TRACERS_MAX_N) { c.err = "tracers: n = " + std::to_string((long long)n) + " outside 1 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); return EKPNP_ERR_INVALID; }
  if (!x || !y || !z) return fail(c, "NULL pointer");
  if (int rc = tracers_check_lattice(c.p, c.err)) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (!tr_position_ok(c.p, x[i], y[i], z[i])) {
      c.err = "tracers: particle " + std::to_string((long long)i) + " at (" + num(x[i]) + ", " + num(y[i]) + ", " + num(z[i]) + ") is outside the lattice";
      return EKPNP_ERR_INVALID;
    }
  const double* const pos[6] = {x, y, z, x, y, z};
  return tracers_upload(c, (long long)n, pos, nullptr, nullptr);
}

extern "C" int ekpnp_tracers_get(ekpnp_ctx* ctx, double* x, double* y, double* z, int32_t* wx, int32_t* wy) {
  NEEDSINGLE(ctx);
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  const TrCloud d = t->dev();
  const size_t n = (size_t)t->n;
  if (x) HIPCHK(c, hipMemcpyAsync(x, d.x, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (y) HIPCHK(c, hipMemcpyAsync(y, d.y, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (z) HIPCHK(c, hipMemcpyAsync(z, d.z, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (wx) HIPCHK(c, hipMemcpyAsync(wx, d.wx, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  if (wy) HIPCHK(c, hipMemcpyAsync(wy, d.wy, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_size(ekpnp_ctx* ctx, int64_t* n) {
  NEEDSINGLE(ctx);
  if (!n) return fail(c, "NULL pointer");
  TracerState* t = cloud_of(c);
  *n = t ? (int64_t)t->n : 0;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_release(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  if (!c.tracers) return EKPNP_OK;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  tracers_release(c);
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_advance(ekpnp_ctx* ctx, double mu, double h, int nsub) {
  NEEDSINGLE(ctx);
  if (int rc = tracers_check_advance(mu, h, nsub, c.err)) return rc;
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  const bool mob = mu != 0.0;
  if (mob)
    if (int rc = ensure_efield(c)) return rc;  // the arrays as ekpnp_get_field would return them (mu == 0: lazy E is left alone)
  const TrFields f{{c.fld[EKPNP_UX], c.fld[EKPNP_UY], c.fld[EKPNP_UZ]}, {c.fld[EKPNP_EX], c.fld[EKPNP_EY], c.fld[EKPNP_EZ]}};
  const TrStep s = tr_step_of(c.p, mu, h, nsub);
  const dim3 grid(tr_blocks(t->n, TR_THREADS)), block(TR_THREADS);
  if (mob) hipLaunchKernelGGL((k_tracers_advance<true>), grid, block, 0, c.stream, f, s, t->dev());
  else hipLaunchKernelGGL((k_tracers_advance<false>), grid, block, 0, c.stream, f, s, t->dev());
  note_launch(c, "k_tracers_advance");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_advance_brownian(ekpnp_ctx* ctx, double mu, double D, double h, int nsub, uint64_t seed) {
  NEEDSINGLE(ctx);
  if (int rc = tracers_check_advance(mu, h, nsub, c.err)) return rc;
  if (int rc = tracers_check_brownian(D, h, c.err)) return rc;
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (t->epoch > INT64_MAX - nsub) { c.err = "tracers: epoch = " + std::to_string((long long)t->epoch) + " (epoch + nsub must fit 63 bits)"; return EKPNP_ERR_INVALID; }
  const bool mob = mu != 0.0;
  if (mob)
    if (int rc = ensure_efield(c)) return rc;  // as ekpnp_tracers_advance (mu == 0: lazy E is left alone)
  const TrFields f{{c.fld[EKPNP_UX], c.fld[EKPNP_UY], c.fld[EKPNP_UZ]}, {c.fld[EKPNP_EX], c.fld[EKPNP_EY], c.fld[EKPNP_EZ]}};
  const TrStep s = tr_step_of(c.p, mu, h, nsub);
  const TrNoise q = tr_noise_of(c.p, D, h, seed, t->epoch);
  const int32_t* ids = t->has_ids ? t->ids : nullptr;
  const dim3 grid(tr_blocks(t->n, TR_THREADS)), block(TR_THREADS);
  if (mob) hipLaunchKernelGGL((k_tracers_advance_brownian<true>), grid, block, 0, c.stream, f, s, q, t->dev(), ids);
  else hipLaunchKernelGGL((k_tracers_advance_brownian<false>), grid, block, 0, c.stream, f, s, q, t->dev(), ids);
  note_launch(c, "k_tracers_advance_brownian");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  t->epoch += nsub;  // every Brownian advance, whether or not particles were lost
  return EKPNP_OK;
}

// the record cleared (enqueues only): epoch -1 and x, y NaN are all bits set (24 B per particle), wall and the image counts 0
static int tracers_land_clear(Ctx& c, TracerState& t) {
  const size_t n = (size_t)t.n;
  HIPCHK(c, hipMemsetAsync(t.land, 0xFF, 24 * n, c.stream));
  HIPCHK(c, hipMemsetAsync((char*)t.land + 24 * n, 0, 12 * n, c.stream));
  return EKPNP_OK;
}

// the record of the cloud, made (and cleared, if asked) on first use
static int tracers_land_alloc(Ctx& c, TracerState& t, bool clear) {
  if (t.land) return EKPNP_OK;
  const size_t bytes = (size_t)t.n * 36;
  HIPCHK(c, hipMalloc(&t.land, bytes));
  t.land_bytes = bytes;
  c.bytes += bytes;
  return clear ? tracers_land_clear(c, t) : EKPNP_OK;
}

extern "C" int ekpnp_tracers_advance_absorbing(ekpnp_ctx* ctx, double mu, double D, double h, int nsub, uint64_t seed, int walls) {
  NEEDSINGLE(ctx);
  if (int rc = tracers_check_advance(mu, h, nsub, c.err)) return rc;
  if (int rc = tracers_check_brownian(D, h, c.err)) return rc;
  if (int rc = tracers_check_walls(walls, c.err)) return rc;
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (t->epoch > INT64_MAX - nsub) { c.err = "tracers: epoch = " + std::to_string((long long)t->epoch) + " (epoch + nsub must fit 63 bits)"; return EKPNP_ERR_INVALID; }
  const bool mob = mu != 0.0;
  if (mob)
    if (int rc = ensure_efield(c)) return rc;  // as ekpnp_tracers_advance (mu == 0: lazy E is left alone)
  if (int rc = tracers_land_alloc(c, *t, true)) return rc;
  const TrFields f{{c.fld[EKPNP_UX], c.fld[EKPNP_UY], c.fld[EKPNP_UZ]}, {c.fld[EKPNP_EX], c.fld[EKPNP_EY], c.fld[EKPNP_EZ]}};
  const TrStep s = tr_step_of(c.p, mu, h, nsub);
  const TrNoise q = tr_noise_of(c.p, D, h, seed, t->epoch);
  const int32_t* ids = t->has_ids ? t->ids : nullptr;
  const dim3 grid(tr_blocks(t->n, TR_THREADS)), block(TR_THREADS);
  if (mob) hipLaunchKernelGGL((k_tracers_advance_absorbing<true>), grid, block, 0, c.stream, f, s, q, walls, t->dev(), ids, t->land_dev());
  else hipLaunchKernelGGL((k_tracers_advance_absorbing<false>), grid, block, 0, c.stream, f, s, q, walls, t->dev(), ids, t->land_dev());
  note_launch(c, "k_tracers_advance_absorbing");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  t->epoch += nsub;  // as a Brownian advance
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_epoch(ekpnp_ctx* ctx, int64_t* epoch) {
  NEEDSINGLE(ctx);
  if (!epoch) return fail(c, "NULL pointer");
  TracerState* t = cloud_of(c);
  *epoch = t ? t->epoch : 0;
  return EKPNP_OK;
}

// ---- the sort ----------------------------------------------------------------------------------------------------------------

static int tracers_ids_alloc(Ctx& c, TracerState& t) {
  if (t.ids) return EKPNP_OK;
  const size_t bytes = (size_t)t.n * sizeof(int32_t);
  HIPCHK(c, hipMalloc((void**)&t.ids, bytes));
  t.ids_bytes = bytes;
  c.bytes += bytes;
  return EKPNP_OK;
}

static inline unsigned ts_runs(long long n) { return (unsigned)((n + TS_RUN - 1) / TS_RUN); }
static inline unsigned ts_chunks(long long n) { return (256u * ts_runs(n) + TS_SCAN - 1) / TS_SCAN; }

extern "C" int ekpnp_tracers_sort(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (int rc = tracers_check_sort_lattice(c.p, c.err)) return rc;
  const long long n = t->n;
  const unsigned nruns = ts_runs(n), chunks = ts_chunks(n);
  if (!t->sort) {  // (16 n is a multiple of 16: the table's uint4 loads are aligned)
    const size_t bytes = 2 * (size_t)n * sizeof(ts_item) + ((size_t)256 * nruns + chunks) * sizeof(unsigned);
    HIPCHK(c, hipMalloc(&t->sort, bytes));
    t->sort_bytes = bytes;
    c.bytes += bytes;
  }
  if (int rc = tracers_ids_alloc(c, *t)) return rc;
  ts_item* a = (ts_item*)t->sort;
  ts_item* b = a + (size_t)n;
  unsigned* hist = (unsigned*)(b + (size_t)n);
  unsigned* sums = hist + (size_t)256 * nruns;
  const TrCloud d = t->dev();
  const dim3 per_particle(tr_blocks(n, TR_THREADS)), block(TR_THREADS);
  hipLaunchKernelGGL(k_tracers_sort_keys, per_particle, block, 0, c.stream, d.x, d.y, d.z, n, c.p.nx, c.p.ny, c.p.nz, a);
  note_launch(c, "k_tracers_sort_keys");
  for (int pass = 0; pass < 4; ++pass) {  // four passes for every lattice: a -> b -> a -> b -> a
    const int shift = 32 + 8 * pass;
    hipLaunchKernelGGL(k_tracers_sort_hist, dim3(nruns), block, 0, c.stream, a, n, shift, nruns, hist);
    note_launch(c, "k_tracers_sort_hist");
    hipLaunchKernelGGL(k_tracers_sort_scan, dim3(chunks), block, 0, c.stream, hist, 256u * nruns, sums);
    note_launch(c, "k_tracers_sort_scan");
    hipLaunchKernelGGL(k_tracers_sort_scan_top, dim3(1), block, 0, c.stream, sums, chunks);
    note_launch(c, "k_tracers_sort_scan_top");
    hipLaunchKernelGGL(k_tracers_sort_scatter, dim3(nruns), block, 0, c.stream, a, b, n, shift, nruns, hist, sums);
    note_launch(c, "k_tracers_sort_scatter");
    ts_item* const s = a;
    a = b;
    b = s;
  }
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  // `a` holds the order, `b` is free: the temporary of the gathers
  double* const arr[6] = {d.x, d.y, d.z, d.x0, d.y0, d.z0};
  for (int q = 0; q < 6; ++q) {
    hipLaunchKernelGGL((k_tracers_sort_gather<double>), per_particle, block, 0, c.stream, a, arr[q], (double*)b, n);
    note_launch(c, "k_tracers_sort_gather");
    HIPCHK(c, hipMemcpyAsync(arr[q], b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
  }
  int32_t* const tmp = (int32_t*)b;  // wx and wy lie behind one another in the cloud: both halves, one copy back
  hipLaunchKernelGGL((k_tracers_sort_gather<int32_t>), per_particle, block, 0, c.stream, a, d.wx, tmp, n);
  note_launch(c, "k_tracers_sort_gather");
  hipLaunchKernelGGL((k_tracers_sort_gather<int32_t>), per_particle, block, 0, c.stream, a, d.wy, tmp + (size_t)n, n);
  note_launch(c, "k_tracers_sort_gather");
  HIPCHK(c, hipMemcpyAsync(d.wx, tmp, 2 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c.stream));
  hipLaunchKernelGGL((k_tracers_sort_gather<int32_t>), per_particle, block, 0, c.stream, a, t->has_ids ? t->ids : nullptr, tmp, n);
  note_launch(c, "k_tracers_sort_gather");
  HIPCHK(c, hipMemcpyAsync(t->ids, tmp, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c.stream));
  if (t->stretch) {  // the stretch record is kept in slot order: its nine F arrays and e go with the particles
    const TrStretch r = t->stretch_dev();
    for (int q = 0; q < 9; ++q) {
      double* const Fq = r.F + (size_t)q * (size_t)n;
      hipLaunchKernelGGL((k_tracers_sort_gather<double>), per_particle, block, 0, c.stream, a, Fq, (double*)b, n);
      note_launch(c, "k_tracers_sort_gather");
      HIPCHK(c, hipMemcpyAsync(Fq, b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    }
    hipLaunchKernelGGL((k_tracers_sort_gather<int32_t>), per_particle, block, 0, c.stream, a, r.e, tmp, n);
    note_launch(c, "k_tracers_sort_gather");
    HIPCHK(c, hipMemcpyAsync(r.e, tmp, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c.stream));
  }
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  t->has_ids = true;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_ids(ekpnp_ctx* ctx, int32_t* id) {
  NEEDSINGLE(ctx);
  if (!id) return fail(c, "NULL pointer");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (!t->has_ids) {  // never sorted: nothing is allocated, nothing is copied
    HIPCHK(c, hipStreamSynchronize(c.stream));
    for (long long i = 0; i < t->n; ++i) id[i] = (int32_t)i;
    return EKPNP_OK;
  }
  HIPCHK(c, hipMemcpyAsync(id, t->ids, (size_t)t->n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

// ---- the cloud's file --------------------------------------------------------------------------------------------------------

namespace {
struct TracerHeader {
  char magic[8];
  int32_t nx, ny, nz, reserved;
  int64_t n;
  double time;
  int64_t reserved2;
};
static_assert(sizeof(TracerHeader) == 48, "tracer file header layout");
constexpr char kTracerMagic[9] = "EKPNPTR1";
}  // namespace

extern "C" int ekpnp_tracers_save(ekpnp_ctx* ctx, const char* path, double time) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  const size_t n = (size_t)t->n;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(c, "cannot open tracer file");
  TracerHeader h{};
  std::memcpy(h.magic, kTracerMagic, 8);
  h.nx = c.p.nx; h.ny = c.p.ny; h.nz = c.p.nz;
  h.n = (int64_t)n;
  h.time = time;
  h.reserved = t->has_ids ? 1 : 0;  // a cloud that was never sorted writes the file it always wrote
  h.reserved2 = t->epoch;           // and so does one that never took a Brownian substep: 0
  bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
  std::vector<double> buf(n);
  const TrCloud d = t->dev();
  const double* const src[6] = {d.x, d.y, d.z, d.x0, d.y0, d.z0};
  for (int a = 0; a < 6 && ok; ++a) {
    if (hipMemcpy(buf.data(), src[a], n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { std::fclose(f); return fail(c, "tracers: copy from the device failed"); }
    ok = std::fwrite(buf.data(), sizeof(double), n, f) == n;
  }
  const int32_t* const wsrc[2] = {d.wx, d.wy};
  for (int a = 0; a < 2 && ok; ++a) {
    if (hipMemcpy(buf.data(), wsrc[a], n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fclose(f); return fail(c, "tracers: copy from the device failed"); }
    ok = std::fwrite(buf.data(), sizeof(int32_t), n, f) == n;
  }
  if (t->has_ids && ok) {
    if (hipMemcpy(buf.data(), t->ids, n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fclose(f); return fail(c, "tracers: copy from the device failed"); }
    ok = std::fwrite(buf.data(), sizeof(int32_t), n, f) == n;
  }
  if (std::fclose(f) != 0 || !ok) return fail(c, "write error on tracer file");
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_load(ekpnp_ctx* ctx, const char* path, double* time) {
  NEEDSINGLE(ctx);
  if (!path || !time) return fail(c, "NULL pointer");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(c, "cannot open tracer file");
  TracerHeader h{};
  if (std::fread(&h, sizeof h, 1, f) != 1 || std::memcmp(h.magic, kTracerMagic, 8) != 0) { std::fclose(f); return fail(c, "tracers: not a tracer file (EKPNPTR1)"); }
  if (h.nx != c.p.nx || h.ny != c.p.ny || h.nz != c.p.nz) {
    std::fclose(f);
    c.err = "tracers: the file holds a cloud of lattice " + std::to_string(h.nx) + " x " + std::to_string(h.ny) + " x " + std::to_string(h.nz) + ", not of " +
            std::to_string(c.p.nx) + " x " + std::to_string(c.p.ny) + " x " + std::to_string(c.p.nz);
    return EKPNP_ERR_INVALID;
  }
  if (h.n < 1 || h.n > EKPNP_TRACERS_MAX_N) { std::fclose(f); c.err = "tracers: n = " + std::to_string((long long)h.n) + " in the file, outside 1 .. " + std::to_string((long long)EKPNP_TRACERS_MAX_N); return EKPNP_ERR_INVALID; }
  if (h.reserved != 0 && h.reserved != 1) { std::fclose(f); c.err = "tracers: reserved = " + std::to_string(h.reserved) + " in the file (0: no ids, 1: ids follow; nothing else is known)"; return EKPNP_ERR_INVALID; }
  if (h.reserved2 < 0) { std::fclose(f); c.err = "tracers: reserved2 = " + std::to_string((long long)h.reserved2) + " in the file (the epoch of the noise: must be >= 0)"; return EKPNP_ERR_INVALID; }
  const size_t n = (size_t)h.n;
  std::vector<double> pos[6];
  std::vector<int32_t> w[2], ids;
  bool ok = true;
  for (int a = 0; a < 6 && ok; ++a) { pos[a].resize(n); ok = std::fread(pos[a].data(), sizeof(double), n, f) == n; }
  for (int a = 0; a < 2 && ok; ++a) { w[a].resize(n); ok = std::fread(w[a].data(), sizeof(int32_t), n, f) == n; }
  if (h.reserved == 1 && ok) { ids.resize(n); ok = std::fread(ids.data(), sizeof(int32_t), n, f) == n; }
  std::fclose(f);
  if (!ok) { c.err = "tracers: the file is shorter than its " + std::to_string((long long)h.n) + " particles"; return EKPNP_ERR_INVALID; }
  for (size_t i = 0; i < n; ++i)
    if (!tr_position_ok(c.p, pos[0][i], pos[1][i], pos[2][i]) || !tr_position_ok(c.p, pos[3][i], pos[4][i], pos[5][i])) {
      c.err = "tracers: particle " + std::to_string(i) + " of the file is outside the lattice";
      return EKPNP_ERR_INVALID;
    }
  const double* const p6[6] = {pos[0].data(), pos[1].data(), pos[2].data(), pos[3].data(), pos[4].data(), pos[5].data()};
  if (h.reserved == 1) {  // the ids must be a permutation of 0 .. n-1
    std::vector<bool> seen(n, false);
    for (size_t s = 0; s < n; ++s) {
      const int32_t v = ids[s];
      if (v < 0 || (size_t)v >= n || seen[(size_t)v]) {
        c.err = "tracers: the ids of the file are not a permutation of 0 .. " + std::to_string(n - 1) + ": slot " + std::to_string(s) + " holds " + std::to_string(v) +
                ((v < 0 || (size_t)v >= n) ? " (out of range)" : " (a second time)");
        return EKPNP_ERR_INVALID;
      }
      seen[(size_t)v] = true;
    }
  }
  if (int rc = tracers_upload(c, (long long)n, p6, w[0].data(), w[1].data())) return rc;
  if (h.reserved == 1) {
    TracerState& t = *c.tracers;
    if (int rc = tracers_ids_alloc(c, t)) return rc;
    HIPCHK(c, hipMemcpy(t.ids, ids.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    t.has_ids = true;
  }
  c.tracers->epoch = h.reserved2;
  *time = h.time;
  return EKPNP_OK;
}

// ---- cell counts and moments -------------------------------------------------------------------------------------------------

// the table of the cell counts, which serves the two reductions of the landing record as well (made by whichever comes first)
static int tracers_cells_alloc(Ctx& c, TracerState& t) {
  if (t.cells) return EKPNP_OK;
  const size_t bytes = ((size_t)EKPNP_TRACERS_MAX_CELLS + 1) * sizeof(unsigned long long);
  HIPCHK(c, hipMalloc((void**)&t.cells, bytes));
  t.cells_bytes = bytes;
  c.bytes += bytes;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_cell_counts(ekpnp_ctx* ctx, int bx, int by, int bz, int64_t* counts, int64_t* lost) {
  NEEDSINGLE(ctx);
  if (!counts || !lost) return fail(c, "NULL pointer");
  if (int rc = tracers_check_cells(c.p, bx, by, bz, c.err)) return rc;
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (int rc = tracers_cells_alloc(c, *t)) return rc;
  const int cells = bx * by * bz;
  HIPCHK(c, hipMemsetAsync(t->cells, 0, ((size_t)cells + 1) * sizeof(unsigned long long), c.stream));
  const TrCloud d = t->dev();
  const dim3 grid(tr_blocks(t->n, TR_THREADS * TR_CELL_PER_THREAD)), block(TR_THREADS);
  if (cells + 1 <= TR_LDS_CELLS)
    hipLaunchKernelGGL((k_tracers_cells<true>), grid, block, ((size_t)cells + 1) * sizeof(unsigned), c.stream, d.x, d.y, d.z, d.n, c.p.nx, c.p.ny, c.p.nz, bx, by, bz, cells, t->cells);
  else
    hipLaunchKernelGGL((k_tracers_cells<false>), grid, block, 0, c.stream, d.x, d.y, d.z, d.n, c.p.nx, c.p.ny, c.p.nz, bx, by, bz, cells, t->cells);
  note_launch(c, "k_tracers_cells");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  std::vector<int64_t> h((size_t)cells + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), t->cells, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  for (int k = 0; k < cells; ++k) counts[k] = h[(size_t)k];
  *lost = h[(size_t)cells];
  return EKPNP_OK;
}

// ---- the landing record: reset, get, the two reductions, the record's file ---------------------------------------------------

static inline TracerState* record_of(Ctx& c) { return c.tracers && c.tracers->cloud && c.tracers->land ? c.tracers : nullptr; }
constexpr const char* kNoRecordMsg = "tracers: no landing record (ekpnp_tracers_advance_absorbing or ekpnp_landings_load makes one)";

extern "C" int ekpnp_landings_reset(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = record_of(c);
  return t ? tracers_land_clear(c, *t) : EKPNP_OK;  // no record: nothing to clear, and nothing is allocated
}

extern "C" int ekpnp_landings_get(ekpnp_ctx* ctx, int64_t* epoch, int32_t* wall, double* x, double* y, int32_t* wx, int32_t* wy) {
  NEEDSINGLE(ctx);
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = record_of(c);
  if (!t) return fail(c, kNoRecordMsg);
  const TrLand d = t->land_dev();
  const size_t n = (size_t)t->n;
  if (epoch) HIPCHK(c, hipMemcpyAsync(epoch, d.epoch, n * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  if (wall) HIPCHK(c, hipMemcpyAsync(wall, d.wall, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  if (x) HIPCHK(c, hipMemcpyAsync(x, d.x, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (y) HIPCHK(c, hipMemcpyAsync(y, d.y, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (wx) HIPCHK(c, hipMemcpyAsync(wx, d.wx, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  if (wy) HIPCHK(c, hipMemcpyAsync(wy, d.wy, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_landings_hist(ekpnp_ctx* ctx, int walls, int64_t e0, int64_t width, int nbins, int64_t* counts, int64_t* none) {
  NEEDSINGLE(ctx);
  if (!counts || !none) return fail(c, "NULL pointer");
  if (int rc = landings_check_hist(walls, e0, width, nbins, c.err)) return rc;
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = record_of(c);
  if (!t) return fail(c, kNoRecordMsg);
  if (int rc = tracers_cells_alloc(c, *t)) return rc;
  const size_t cells = (size_t)nbins + 2;
  HIPCHK(c, hipMemsetAsync(t->cells, 0, (cells + 1) * sizeof(unsigned long long), c.stream));
  const TrLand d = t->land_dev();
  hipLaunchKernelGGL(k_landings_hist, dim3(tr_blocks(t->n, TR_THREADS * TR_CELL_PER_THREAD)), dim3(TR_THREADS), (cells + 1) * sizeof(unsigned), c.stream, d.epoch, d.wall, t->n,
                     walls, e0, width, nbins, t->cells);
  note_launch(c, "k_landings_hist");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  std::vector<int64_t> h(cells + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), t->cells, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  for (size_t k = 0; k < cells; ++k) counts[k] = h[k];
  *none = h[cells];
  return EKPNP_OK;
}

extern "C" int ekpnp_landings_map(ekpnp_ctx* ctx, int wall, int bx, int by, int64_t e_lo, int64_t e_hi, int64_t* counts, int64_t* elsewhere) {
  NEEDSINGLE(ctx);
  if (!counts || !elsewhere) return fail(c, "NULL pointer");
  if (wall < 1 || wall > 2) { c.err = "tracers: wall = " + std::to_string(wall) + " (must be 1, the bottom plate, or 2, the top plate)"; return EKPNP_ERR_INVALID; }
  if (int rc = tracers_check_cells(c.p, bx, by, 1, c.err)) return rc;
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = record_of(c);
  if (!t) return fail(c, kNoRecordMsg);
  if (int rc = tracers_cells_alloc(c, *t)) return rc;
  const int cells = bx * by;
  HIPCHK(c, hipMemsetAsync(t->cells, 0, ((size_t)cells + 1) * sizeof(unsigned long long), c.stream));
  const dim3 grid(tr_blocks(t->n, TR_THREADS * TR_CELL_PER_THREAD)), block(TR_THREADS);
  if (cells + 1 <= TR_LDS_CELLS)
    hipLaunchKernelGGL((k_landings_map<true>), grid, block, ((size_t)cells + 1) * sizeof(unsigned), c.stream, t->land_dev(), t->n, wall, e_lo, e_hi, c.p.nx, c.p.ny, c.p.nz, bx, by, cells, t->cells);
  else
    hipLaunchKernelGGL((k_landings_map<false>), grid, block, 0, c.stream, t->land_dev(), t->n, wall, e_lo, e_hi, c.p.nx, c.p.ny, c.p.nz, bx, by, cells, t->cells);
  note_launch(c, "k_landings_map");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  std::vector<int64_t> h((size_t)cells + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), t->cells, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  for (int k = 0; k < cells; ++k) counts[k] = h[(size_t)k];
  *elsewhere = h[(size_t)cells];
  return EKPNP_OK;
}

namespace {
struct LandHeader {
  char magic[8];
  int32_t nx, ny, nz, reserved;
  int64_t n, landed, epoch;
};
static_assert(sizeof(LandHeader) == 48, "landing file header layout");
constexpr char kLandMagic[9] = "EKPNPLD1";
}  // namespace

extern "C" int ekpnp_landings_save(ekpnp_ctx* ctx, const char* path) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = record_of(c);
  if (!t) return fail(c, kNoRecordMsg);
  const size_t n = (size_t)t->n;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  std::vector<int64_t> buf((36 * n + 7) / 8);  // the record lies in memory as in the file
  HIPCHK(c, hipMemcpy(buf.data(), t->land, 36 * n, hipMemcpyDeviceToHost));
  const int32_t* wall = (const int32_t*)((const char*)buf.data() + 24 * n);
  LandHeader h{};
  std::memcpy(h.magic, kLandMagic, 8);
  h.nx = c.p.nx; h.ny = c.p.ny; h.nz = c.p.nz;
  h.n = (int64_t)n;
  h.epoch = t->epoch;
  for (size_t i = 0; i < n; ++i) h.landed += wall[i] != 0;
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(c, "cannot open landing file");
  const bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && std::fwrite(buf.data(), 1, 36 * n, f) == 36 * n;
  if (std::fclose(f) != 0 || !ok) return fail(c, "write error on landing file");
  return EKPNP_OK;
}

extern "C" int ekpnp_landings_load(ekpnp_ctx* ctx, const char* path) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(c, "cannot open landing file");
  LandHeader h{};
  if (std::fread(&h, sizeof h, 1, f) != 1 || std::memcmp(h.magic, kLandMagic, 8) != 0) { std::fclose(f); return fail(c, "tracers: not a landing file (EKPNPLD1)"); }
  if (h.nx != c.p.nx || h.ny != c.p.ny || h.nz != c.p.nz) {
    std::fclose(f);
    c.err = "tracers: the file holds a landing record of lattice " + std::to_string(h.nx) + " x " + std::to_string(h.ny) + " x " + std::to_string(h.nz) + ", not of " +
            std::to_string(c.p.nx) + " x " + std::to_string(c.p.ny) + " x " + std::to_string(c.p.nz);
    return EKPNP_ERR_INVALID;
  }
  if (h.n != (int64_t)t->n) { std::fclose(f); c.err = "tracers: n = " + std::to_string((long long)h.n) + " in the landing file, the cloud has " + std::to_string(t->n) + " particles"; return EKPNP_ERR_INVALID; }
  if (h.reserved != 0) { std::fclose(f); c.err = "tracers: reserved = " + std::to_string(h.reserved) + " in the landing file (must be 0)"; return EKPNP_ERR_INVALID; }
  if (h.epoch < 0) { std::fclose(f); c.err = "tracers: epoch = " + std::to_string((long long)h.epoch) + " in the landing file (must be >= 0)"; return EKPNP_ERR_INVALID; }
  const size_t n = (size_t)h.n;
  std::vector<int64_t> buf((36 * n + 7) / 8);
  const bool ok = std::fread(buf.data(), 1, 36 * n, f) == 36 * n;
  std::fclose(f);
  if (!ok) { c.err = "tracers: the landing file is shorter than its " + std::to_string((long long)h.n) + " entries"; return EKPNP_ERR_INVALID; }
  const int64_t* epoch = buf.data();
  const int32_t* wall = (const int32_t*)((const char*)buf.data() + 24 * n);
  int64_t landed = 0;
  for (size_t i = 0; i < n; ++i) {
    const std::string w = "tracers: landing file, id " + std::to_string(i) + ": ";
    if (wall[i] < 0 || wall[i] > 2) { c.err = w + "wall = " + std::to_string(wall[i]) + " outside 0 .. 2"; return EKPNP_ERR_INVALID; }
    if (epoch[i] < -1 || (epoch[i] == -1) != (wall[i] == 0)) {
      c.err = w + "epoch = " + std::to_string((long long)epoch[i]) + " with wall = " + std::to_string(wall[i]) + " (epoch -1 and wall 0 go together: no landing)";
      return EKPNP_ERR_INVALID;
    }
    if (epoch[i] > h.epoch) { c.err = w + "epoch = " + std::to_string((long long)epoch[i]) + " above the file's epoch " + std::to_string((long long)h.epoch); return EKPNP_ERR_INVALID; }
    landed += wall[i] != 0;
  }
  if (landed != h.landed) { c.err = "tracers: landed = " + std::to_string((long long)h.landed) + " in the landing file, which holds " + std::to_string((long long)landed) + " entries with a wall"; return EKPNP_ERR_INVALID; }
  HIPCHK(c, hipStreamSynchronize(c.stream));  // an absorbing advance may still write the record
  if (int rc = tracers_land_alloc(c, *t, false)) return rc;
  HIPCHK(c, hipMemcpy(t->land, buf.data(), 36 * n, hipMemcpyHostToDevice));
  return EKPNP_OK;
}

// ---- the stretch record: begin, end, the tangent advance, get, the histogram of levels, the record's file ----------------------

static inline TracerState* stretch_of(Ctx& c) { return c.tracers && c.tracers->cloud && c.tracers->stretch ? c.tracers : nullptr; }
constexpr const char* kNoStretchMsg = "tracers: no stretch record (ekpnp_tracers_stretch_begin or ekpnp_tracers_stretch_load makes one)";

static int tracers_stretch_alloc(Ctx& c, TracerState& t) {
  if (t.stretch) return EKPNP_OK;
  const size_t bytes = (size_t)t.n * 76;
  HIPCHK(c, hipMalloc(&t.stretch, bytes));
  t.stretch_bytes = bytes;
  c.bytes += bytes;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_stretch_begin(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (int rc = tracers_stretch_alloc(c, *t)) return rc;
  const TrCloud d = t->dev();
  hipLaunchKernelGGL(k_stretch_begin, dim3(tr_blocks(t->n, TR_THREADS)), dim3(TR_THREADS), 0, c.stream, d.x, d.y, d.z, t->n, t->stretch_dev());
  note_launch(c, "k_stretch_begin");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_stretch_end(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  if (!c.tracers) return EKPNP_OK;
  return tracers_stretch_drop(c, *c.tracers);
}

extern "C" int ekpnp_tracers_advance_tangent(ekpnp_ctx* ctx, double mu, double h, int nsub) {
  NEEDSINGLE(ctx);
  if (int rc = tracers_check_advance(mu, h, nsub, c.err)) return rc;
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = stretch_of(c);
  if (!t) return fail(c, kNoStretchMsg);
  const bool mob = mu != 0.0;
  if (mob)
    if (int rc = ensure_efield(c)) return rc;  // as ekpnp_tracers_advance (mu == 0: lazy E is left alone)
  const TrFields f{{c.fld[EKPNP_UX], c.fld[EKPNP_UY], c.fld[EKPNP_UZ]}, {c.fld[EKPNP_EX], c.fld[EKPNP_EY], c.fld[EKPNP_EZ]}};
  const TrStep s = tr_step_of(c.p, mu, h, nsub);
  const dim3 grid(tr_blocks(t->n, TR_THREADS)), block(TR_THREADS);
  if (mob) hipLaunchKernelGGL((k_tracers_advance_tangent<true>), grid, block, 0, c.stream, f, s, t->dev(), t->stretch_dev());
  else hipLaunchKernelGGL((k_tracers_advance_tangent<false>), grid, block, 0, c.stream, f, s, t->dev(), t->stretch_dev());
  note_launch(c, "k_tracers_advance_tangent");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_stretch_get(ekpnp_ctx* ctx, double* F, int32_t* e) {
  NEEDSINGLE(ctx);
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = stretch_of(c);
  if (!t) return fail(c, kNoStretchMsg);
  const TrStretch r = t->stretch_dev();
  const size_t n = (size_t)t->n;
  if (F) HIPCHK(c, hipMemcpyAsync(F, r.F, 9 * n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  if (e) HIPCHK(c, hipMemcpyAsync(e, r.e, n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_stretch_levels(ekpnp_ctx* ctx, int l_lo, int nlevels, int64_t* counts, int64_t* none) {
  NEEDSINGLE(ctx);
  if (!counts || !none) return fail(c, "NULL pointer");
  if (nlevels < 1 || nlevels > 4096) { c.err = "tracers: nlevels = " + std::to_string(nlevels) + " outside 1 .. 4096"; return EKPNP_ERR_INVALID; }
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = stretch_of(c);
  if (!t) return fail(c, kNoStretchMsg);
  if (int rc = tracers_cells_alloc(c, *t)) return rc;
  const size_t cells = (size_t)nlevels + 2;
  HIPCHK(c, hipMemsetAsync(t->cells, 0, (cells + 1) * sizeof(unsigned long long), c.stream));
  hipLaunchKernelGGL(k_stretch_levels, dim3(tr_blocks(t->n, TR_THREADS * TR_CELL_PER_THREAD)), dim3(TR_THREADS), (cells + 1) * sizeof(unsigned), c.stream, t->stretch_dev(), t->n,
                     l_lo, nlevels, t->cells);
  note_launch(c, "k_stretch_levels");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  std::vector<int64_t> h(cells + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), t->cells, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  for (size_t k = 0; k < cells; ++k) counts[k] = h[k];
  *none = h[cells];
  return EKPNP_OK;
}

namespace {
struct StretchHeader {
  char magic[8];
  int32_t nx, ny, nz, reserved;
  int64_t n, reserved2, reserved3;
};
static_assert(sizeof(StretchHeader) == 48, "stretch file header layout");
constexpr char kStretchMagic[9] = "EKPNPSF1";
}  // namespace

extern "C" int ekpnp_tracers_stretch_save(ekpnp_ctx* ctx, const char* path) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  if (!cloud_of(c)) return fail(c, "tracers: no cloud (seed, set or load one first)");
  TracerState* t = stretch_of(c);
  if (!t) return fail(c, kNoStretchMsg);
  const size_t n = (size_t)t->n;
  HIPCHK(c, hipStreamSynchronize(c.stream));
  std::vector<double> buf((76 * n + 7) / 8);  // in memory F comes first, in the file e
  HIPCHK(c, hipMemcpy(buf.data(), t->stretch, 76 * n, hipMemcpyDeviceToHost));
  StretchHeader h{};
  std::memcpy(h.magic, kStretchMagic, 8);
  h.nx = c.p.nx; h.ny = c.p.ny; h.nz = c.p.nz;
  h.n = (int64_t)n;
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(c, "cannot open stretch file");
  const bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && std::fwrite((const char*)buf.data() + 72 * n, 1, 4 * n, f) == 4 * n && std::fwrite(buf.data(), 1, 72 * n, f) == 72 * n;
  if (std::fclose(f) != 0 || !ok) return fail(c, "write error on stretch file");
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_stretch_load(ekpnp_ctx* ctx, const char* path) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(c, "cannot open stretch file");
  StretchHeader h{};
  if (std::fread(&h, sizeof h, 1, f) != 1 || std::memcmp(h.magic, kStretchMagic, 8) != 0) { std::fclose(f); return fail(c, "tracers: not a stretch file (EKPNPSF1)"); }
  if (h.nx != c.p.nx || h.ny != c.p.ny || h.nz != c.p.nz) {
    std::fclose(f);
    c.err = "tracers: the file holds a stretch record of lattice " + std::to_string(h.nx) + " x " + std::to_string(h.ny) + " x " + std::to_string(h.nz) + ", not of " +
            std::to_string(c.p.nx) + " x " + std::to_string(c.p.ny) + " x " + std::to_string(c.p.nz);
    return EKPNP_ERR_INVALID;
  }
  if (h.n != (int64_t)t->n) { std::fclose(f); c.err = "tracers: n = " + std::to_string((long long)h.n) + " in the stretch file, the cloud has " + std::to_string(t->n) + " particles"; return EKPNP_ERR_INVALID; }
  if (h.reserved != 0 || h.reserved2 != 0 || h.reserved3 != 0) {
    std::fclose(f);
    c.err = "tracers: reserved = " + std::to_string(h.reserved) + ", " + std::to_string((long long)h.reserved2) + ", " + std::to_string((long long)h.reserved3) + " in the stretch file (must be 0)";
    return EKPNP_ERR_INVALID;
  }
  const size_t n = (size_t)h.n;
  std::vector<double> buf((76 * n + 7) / 8);
  const bool ok = std::fread((char*)buf.data() + 72 * n, 1, 4 * n, f) == 4 * n && std::fread(buf.data(), 1, 72 * n, f) == 72 * n;
  std::fclose(f);
  if (!ok) { c.err = "tracers: the stretch file is shorter than its " + std::to_string((long long)h.n) + " entries"; return EKPNP_ERR_INVALID; }
  HIPCHK(c, hipStreamSynchronize(c.stream));  // a tangent advance may still write the record
  if (int rc = tracers_stretch_alloc(c, *t)) return rc;
  HIPCHK(c, hipMemcpy(t->stretch, buf.data(), 76 * n, hipMemcpyHostToDevice));
  return EKPNP_OK;
}

// enqueue the 12 moments of the cloud into `out` (device memory)
static int tracers_enqueue_moments(Ctx& c, TracerState& t, double* out) {
  hipLaunchKernelGGL(k_tracers_partials, dim3(t.nwg), dim3(TR_THREADS), 0, c.stream, t.dev(), c.p.nx, c.p.ny, t.part);
  note_launch(c, "k_tracers_partials");
  hipLaunchKernelGGL(k_tracers_finish, dim3(1), dim3(64), 0, c.stream, t.part, t.nwg, out);
  note_launch(c, "k_tracers_finish");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_moments(ekpnp_ctx* ctx, double* out) {
  NEEDSINGLE(ctx);
  if (!out) return fail(c, "NULL pointer");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (int rc = tracers_enqueue_moments(c, *t, t->out())) return rc;
  HIPCHK(c, hipMemcpyAsync(out, t->out(), NM * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

// ---- the time series ---------------------------------------------------------------------------------------------------------

extern "C" int ekpnp_tracers_arm(ekpnp_ctx* ctx, int capacity) {
  NEEDSINGLE(ctx);
  if (capacity < 1) { c.err = "tracers: capacity = " + std::to_string(capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  if (int rc = need_tracers(c)) return rc;
  return ring_arm(c, c.tracers->ring, capacity, NM * sizeof(double));
}

extern "C" int ekpnp_tracers_disarm(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  if (c.tracers) c.tracers->ring.armed = false;  // the ring and its rows stay readable until the next arm
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDSINGLE(ctx);
  if (!c.tracers || !c.tracers->ring.armed) return fail(c, "ekpnp_tracers_record: no ring armed");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (int rc = tracers_enqueue_moments(c, *t, (double*)ring_next_row(t->ring))) return rc;
  ring_note_row(t->ring, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_count(ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  NEEDSINGLE(ctx);
  ring_count(c.tracers ? &c.tracers->ring : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, double* values) {
  NEEDSINGLE(ctx);
  return ring_read(c, c.tracers ? &c.tracers->ring : nullptr, "ekpnp_tracers_read", first, count, steps, times, values);
}

extern "C" int ekpnp_tracers_ring_save(ekpnp_ctx* ctx, const char* path) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  if (!c.tracers || !c.tracers->ring.ever_armed) return fail(c, "ekpnp_tracers_ring_save: no ring was armed");
  int64_t rec = 0, dropped = 0;
  ring_count(&c.tracers->ring, &rec, &dropped);
  const int n = (int)(rec - dropped);
  std::vector<int64_t> steps((size_t)n);
  std::vector<double> times((size_t)n), values((size_t)n * NM);
  if (int rc = ring_read(c, &c.tracers->ring, "ekpnp_tracers_ring_save", 0, n, steps.data(), times.data(), values.data())) return rc;
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(c, "cannot open tracers file");
  std::fprintf(f, "# ekpnp tracers nx %d ny %d nz %d n %lld recorded %lld dropped %lld\n", c.p.nx, c.p.ny, c.p.nz, (long long)c.tracers->n, (long long)rec, (long long)dropped);
  std::fprintf(f, "# step time");
  for (int q = 0; q < NM; ++q) std::fprintf(f, " %s", kMomentNames[q]);
  std::fprintf(f, "\n");
  for (int r = 0; r < n; ++r) {
    std::fprintf(f, "%lld %.17g", (long long)steps[(size_t)r], times[(size_t)r]);
    for (int q = 0; q < NM; ++q) std::fprintf(f, " %.17g", values[(size_t)r * NM + q]);
    std::fprintf(f, "\n");
  }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) return fail(c, "write error on tracers file");
  return EKPNP_OK;
}

// ---- the fields at the particles ---------------------------------------------------------------------------------------------

// enqueue the sample of a checked list of values into `out` (device memory, [nvalues][n])
static int tracers_enqueue_sample(Ctx& c, TracerState& t, int nvalues, const int32_t* values, double* out) {
  if (tr_names_phi_or_e(nvalues, values))
    if (int rc = ensure_efield(c)) return rc;  // the arrays as ekpnp_get_field would return them (otherwise lazy E is left alone)
  const TrSample a = tr_sample_plan(c.p, nvalues, values, c.fld);
  const TrCloud d = t.dev();
  hipLaunchKernelGGL(k_tracers_sample, dim3(tr_blocks(t.n, TR_THREADS)), dim3(TR_THREADS), 0, c.stream, a, d.x, d.y, d.z, d.n, out);
  note_launch(c, "k_tracers_sample");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracers_sample_device(ekpnp_ctx* ctx, int nvalues, const int32_t* values, double* device_out) {
  NEEDSINGLE(ctx);
  if (!values || !device_out) return fail(c, "NULL pointer");
  if (int rc = tracers_check_values(c.p, nvalues, values, 1, c.err)) return rc;
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  return tracers_enqueue_sample(c, *t, nvalues, values, device_out);
}

extern "C" int ekpnp_tracers_sample(ekpnp_ctx* ctx, int nvalues, const int32_t* values, double* host_out) {
  NEEDSINGLE(ctx);
  if (!values || !host_out) return fail(c, "NULL pointer");
  if (int rc = tracers_check_values(c.p, nvalues, values, 1, c.err)) return rc;
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  const size_t bytes = (size_t)nvalues * (size_t)t->n * sizeof(double);
  if (bytes > t->samp_bytes) {
    HIPCHK(c, hipStreamSynchronize(c.stream));  // an earlier sample may still write the old scratch
    if (t->samp) { (void)hipFree(t->samp); c.bytes -= t->samp_bytes; t->samp = nullptr; t->samp_bytes = 0; }
    HIPCHK(c, hipMalloc((void**)&t->samp, bytes));
    t->samp_bytes = bytes;
    c.bytes += bytes;
  }
  if (int rc = tracers_enqueue_sample(c, *t, nvalues, values, t->samp)) return rc;
  HIPCHK(c, hipMemcpyAsync(host_out, t->samp, bytes, hipMemcpyDeviceToHost, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));
  return EKPNP_OK;
}

// ---- tracks of tagged particles ----------------------------------------------------------------------------------------------

static inline size_t tracks_header_bytes(int ntags) { return (((size_t)4 * ntags * sizeof(int32_t)) + 15) & ~(size_t)15; }
static inline int tracks_row_doubles(const ekpnp_tracks_spec& s) { return s.ntags * (5 + s.nvalues); }
static TrTags tracks_tags(const TracerState& t) {
  int32_t* h = (int32_t*)t.tracks.alloc;
  const int m = t.tspec.ntags;
  return TrTags{h, h + m, h + 2 * m, h + 3 * m, m};
}

extern "C" int ekpnp_tracks_arm(ekpnp_ctx* ctx, const ekpnp_tracks_spec* spec, int capacity) {
  NEEDSINGLE(ctx);
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  if (int rc = tracers_check_tracks(c.p, (int64_t)t->n, spec, c.err)) return rc;
  if (capacity < 1) { c.err = "tracers: capacity = " + std::to_string(capacity) + " (must be >= 1)"; return EKPNP_ERR_INVALID; }
  const int m = spec->ntags;
  if (int rc = ring_arm(c, t->tracks, capacity, (size_t)tracks_row_doubles(*spec) * sizeof(double), tracks_header_bytes(m))) return rc;
  t->tracks.armed = false;  // until the tables have landed
  t->tspec = *spec;
  t->tracks_n = t->n;
  // the header: ids as given | ids ascending | the place of each of those | the slots (zeros until the first find)
  std::vector<int32_t> tab((size_t)3 * m);
  std::vector<std::pair<int32_t, int32_t>> byid((size_t)m);
  for (int k = 0; k < m; ++k) byid[(size_t)k] = {spec->ids[k], k};
  std::sort(byid.begin(), byid.end());
  for (int k = 0; k < m; ++k) {
    tab[(size_t)k] = spec->ids[k];
    tab[(size_t)m + k] = byid[(size_t)k].first;
    tab[(size_t)2 * m + k] = byid[(size_t)k].second;
  }
  HIPCHK(c, hipMemcpyAsync(t->tracks.alloc, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
  HIPCHK(c, hipStreamSynchronize(c.stream));  // `tab` goes away
  t->tracks.armed = true;
  return EKPNP_OK;
}

extern "C" int ekpnp_tracks_disarm(ekpnp_ctx* ctx) {
  NEEDSINGLE(ctx);
  if (c.tracers) c.tracers->tracks.armed = false;  // the ring and its rows stay readable until the next arm
  return EKPNP_OK;
}

extern "C" int ekpnp_tracks_record(ekpnp_ctx* ctx, int64_t step, double time) {
  NEEDSINGLE(ctx);
  if (!c.tracers || !c.tracers->tracks.armed) return fail(c, "ekpnp_tracks_record: no ring armed");
  TracerState* t = cloud_of(c);
  if (!t) return fail(c, "tracers: no cloud (seed, set or load one first)");
  const ekpnp_tracks_spec& s = t->tspec;
  if (tr_names_phi_or_e(s.nvalues, s.values))
    if (int rc = ensure_efield(c)) return rc;
  const TrTags tags = tracks_tags(*t);
  if (t->has_ids) {  // a sorted cloud: where is each tagged particle now?
    const long long quads = (t->n + TK_IDS - 1) / TK_IDS;
    hipLaunchKernelGGL(k_tracers_track_find, dim3(tr_blocks(quads, TR_THREADS)), dim3(TR_THREADS), 0, c.stream, t->ids, t->n, tags);
    note_launch(c, "k_tracers_track_find");
  }
  const TrSample a = tr_sample_plan(c.p, s.nvalues, s.values, c.fld);
  hipLaunchKernelGGL(k_tracers_track_row, dim3(tr_blocks(s.ntags, TR_THREADS)), dim3(TR_THREADS), 0, c.stream, a, t->dev(), tags,
                     t->has_ids ? (const int32_t*)tags.slot : (const int32_t*)nullptr, (double*)ring_next_row(t->tracks));
  note_launch(c, "k_tracers_track_row");
  if (take_launch_error(c) != hipSuccess) return EKPNP_ERR_HIP;
  ring_note_row(t->tracks, step, time);
  return EKPNP_OK;
}

extern "C" int ekpnp_tracks_count(ekpnp_ctx* ctx, int64_t* recorded, int64_t* dropped) {
  NEEDSINGLE(ctx);
  ring_count(c.tracers ? &c.tracers->tracks : nullptr, recorded, dropped);
  return EKPNP_OK;
}

extern "C" int ekpnp_tracks_read(ekpnp_ctx* ctx, int64_t first, int count, int64_t* steps, double* times, double* values) {
  NEEDSINGLE(ctx);
  return ring_read(c, c.tracers ? &c.tracers->tracks : nullptr, "ekpnp_tracks_read", first, count, steps, times, values);
}

extern "C" int ekpnp_tracks_save(ekpnp_ctx* ctx, const char* path) {
  NEEDSINGLE(ctx);
  if (!path) return fail(c, "NULL path");
  if (!c.tracers || !c.tracers->tracks.ever_armed || !c.tracers->tracks.alloc) return fail(c, "ekpnp_tracks_save: no ring was armed");
  const TracerState& t = *c.tracers;
  const ekpnp_tracks_spec& s = t.tspec;
  int64_t rec = 0, dropped = 0;
  ring_count(&t.tracks, &rec, &dropped);
  const int n = (int)(rec - dropped), w = 5 + s.nvalues;
  std::vector<int64_t> steps((size_t)n);
  std::vector<double> times((size_t)n), values((size_t)n * (size_t)tracks_row_doubles(s));
  if (int rc = ring_read(c, &t.tracks, "ekpnp_tracks_save", 0, n, steps.data(), times.data(), values.data())) return rc;
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(c, "cannot open tracks file");
  std::fprintf(f, "# ekpnp tracks nx %d ny %d nz %d n %lld ntags %d nvalues %d recorded %lld dropped %lld\n", c.p.nx, c.p.ny, c.p.nz, t.tracks_n, s.ntags, s.nvalues,
               (long long)rec, (long long)dropped);
  std::fprintf(f, "# step time id x y z wx wy");
  for (int v = 0; v < s.nvalues; ++v) std::fprintf(f, " %s", kValueNames[s.values[v]]);
  std::fprintf(f, "\n");
  for (int r = 0; r < n; ++r)
    for (int k = 0; k < s.ntags; ++k) {
      const double* q = values.data() + ((size_t)r * s.ntags + k) * w;
      std::fprintf(f, "%lld %.17g %d %.17g %.17g %.17g %d %d", (long long)steps[(size_t)r], times[(size_t)r], s.ids[k], q[0], q[1], q[2], (int)q[3], (int)q[4]);
      for (int v = 0; v < s.nvalues; ++v) std::fprintf(f, " %.17g", q[5 + v]);
      std::fprintf(f, "\n");
    }
  const bool bad = std::ferror(f) != 0;
  if (std::fclose(f) != 0 || bad) return fail(c, "write error on tracks file");
  return EKPNP_OK;
}
