// plan_check.cpp — csrc/launch_plan.h against the predicates it replaced (tests/test_plan_cpu.py builds and runs it).
// The model below is those predicates as the launchers spelled them before the header existed - the two `if` chains of the z
// solve with their launch macros, slab_part_modes, slab_read_once, tridiag_is_partition, both block functions with their counts,
// the per_xcd formula and the (NL > 1) rule - transcribed literally onto a struct that holds the fields of the context they read.
// Prints "ok <cases>" and returns 0, or the first mismatch and 1.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ek-pnp-3d_amd/csrc/launch_plan.h"

using namespace ekpnp;

#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAILED " __VA_ARGS__); \
      std::printf(" [%s]\n", #cond);      \
      return 1;                           \
    }                                     \
  } while (0)

// ---- the model ---------------------------------------------------------------------------------------------------------------
namespace model {

struct Params {
  int ny, nz, n_lattices;
};
struct Ctx {
  Params p;
  int nxh, slab_m, tri_partition, edge_chunks, poisson_blocks, nranks;
  bool tri_lds_ok, slab, own_fft, streamed_state;
};
struct double2 {
  double x, y;
};
struct ModeBlock {
  int x0, bw;
  size_t local_off, all_off, doubles;
};
constexpr int TRI_THREADS = 64;

// what a branch of a chain launched: kernel family, template arguments, modes per workgroup (the grid's divisor), dynamic LDS, name
struct Launch {
  ZFamily family;
  int R, lanes, group, lds;
  const char* name;
};

// launch_tridiag
#define TRI_PART(RR, LL, GROUP, NAME) \
  Launch { ZFamily::partition, RR, LL, GROUP, (RR) * 8192, "k_tridiag_part<" NAME ">" }
static Launch launch_tridiag(const Ctx& c) {
  const int nm = c.p.ny * c.nxh;
  const bool part = c.tri_partition > 0 && c.tri_lds_ok && c.nxh % 8 == 0;
  const int rows = c.p.nz - 2;
  const bool large = c.tri_partition > 1 || (size_t)nm * (size_t)rows >= (size_t)4 * 1024 * 1024;
  if (rows <= 64) {
    return Launch{ZFamily::pcr64, 1, 64, 4, 0, "k_tridiag_pcr64"};  // dim3((nm + 3) / 4), dim3(256), 0
  } else if (part && large && rows <= 128 && nm % 32 == 0) {
    return TRI_PART(8, 16, 32, "8,16");
  } else if (part && large && rows <= 256 && nm % 16 == 0) {
    return TRI_PART(8, 32, 16, "8,32");
  } else if (part && large && rows <= 256) {
    return TRI_PART(4, 64, 8, "4");
  } else if (part && large && rows <= 512) {
    return TRI_PART(8, 64, 8, "8");
  } else {
    return Launch{ZFamily::serial, 0, 1, TRI_THREADS, 0, "k_tridiag"};  // dim3((nm + TRI_THREADS - 1) / TRI_THREADS), dim3(TRI_THREADS), 0
  }
}
#undef TRI_PART

static inline bool slab_read_once(const Ctx& c) { return c.tri_partition > 0 && c.tri_lds_ok && c.nxh % 8 == 0 && c.slab_m >= 1 && c.slab_m <= 512; }
static int slab_part_modes(const Ctx& c) {
  const int m = c.slab_m, nm = c.p.ny * c.nxh;
  if (m <= 128) return nm % 32 == 0 ? 32 : 8;
  if (m <= 256) return nm % 16 == 0 ? 16 : 8;
  return 8;
}
// launch_slab_reduce_correct (after k_slab_interface)
#define SLAB_PART(RR, LL, GROUP, NAME) \
  return Launch { ZFamily::partition, RR, LL, GROUP, (RR) * 8192, "k_slab_part<" NAME ">" }
static Launch launch_slab_reduce_correct(const Ctx& c) {
  if (slab_read_once(c)) {
    const int m = c.slab_m;
    const int mc = slab_part_modes(c);
    if (m <= 128 && mc == 32) SLAB_PART(8, 16, 32, "8,16");
    else if (m <= 128) SLAB_PART(2, 64, 8, "2");
    else if (m <= 256 && mc == 16) SLAB_PART(8, 32, 16, "8,32");
    else if (m <= 256) SLAB_PART(4, 64, 8, "4");
    else SLAB_PART(8, 64, 8, "8");
  }
  return Launch{ZFamily::slab_serial, 0, 1, 64, 0, "k_slab_reduce_correct"};  // dim3((nm + 63) / 64), dim3(64), 0
}
#undef SLAB_PART
// launch_slab_thomas_local: k_slab_edges (true) or k_slab_thomas_local
static bool stage1_is_slab_edges(const Ctx& c) { return slab_read_once(c); }

static int gcd_int(int a, int b) { return b == 0 ? a : gcd_int(b, a % b); }
static int block_unit_groups(const Ctx& c) {
  if (c.nxh % 8 != 0) return 1;
  return 4 / gcd_int(4, c.p.ny);
}
static int edge_chunk_count(const Ctx& c) {
  if (c.nxh % 8 != 0) return 1;
  const int gu = block_unit_groups(c), units = (c.nxh / 8 + gu - 1) / gu;
  return c.edge_chunks < 1 ? 1 : (c.edge_chunks > units ? units : c.edge_chunks);
}
static ModeBlock mode_block(const Ctx& c, int k) {
  ModeBlock b;
  if (c.nxh % 8 != 0) {
    b.x0 = 0;
    b.bw = c.nxh;
  } else {
    const int groups = c.nxh / 8, gu = block_unit_groups(c), units = (groups + gu - 1) / gu, nb = edge_chunk_count(c);
    const int u0 = (int)((long long)units * k / nb), u1 = (int)((long long)units * (k + 1) / nb);
    const int g0 = u0 * gu, g1 = u1 * gu < groups ? u1 * gu : groups;
    b.x0 = g0 * 8;
    b.bw = (g1 - g0) * 8;
  }
  b.local_off = (size_t)4 * c.p.ny * b.x0;
  b.all_off = (size_t)c.nranks * 4 * c.p.ny * b.x0;
  b.doubles = (size_t)4 * c.p.ny * b.bw;
  return b;
}

static bool tridiag_is_partition(const Ctx& c) {
  const int nm = c.p.ny * c.nxh, rows = c.p.nz - 2;
  const bool part = c.tri_partition > 0 && c.tri_lds_ok && c.nxh % 8 == 0;
  const bool large = c.tri_partition > 1 || (size_t)nm * (size_t)rows >= (size_t)4 * 1024 * 1024;
  return part && large && rows > 64 && rows <= 512;
}
static int poisson_block_count(const Ctx& c) {
  if (c.slab || !c.own_fft || c.poisson_blocks == 1 || !tridiag_is_partition(c)) return 1;
  int want = c.poisson_blocks;
  if (want <= 0) want = (size_t)c.p.ny * c.nxh * (size_t)(c.p.nz - 2) * sizeof(double2) >= ((size_t)768 << 20) ? 3 : 1;
  const int gu = block_unit_groups(c), units = (c.nxh / 8 + gu - 1) / gu;
  return want > units ? units : want;
}
static ModeBlock poisson_block(const Ctx& c, int k) {
  ModeBlock b{};
  const int groups = c.nxh / 8, gu = block_unit_groups(c), units = (groups + gu - 1) / gu, nb = poisson_block_count(c);
  const int u0 = (int)((long long)units * k / nb), u1 = (int)((long long)units * (k + 1) / nb);
  const int g0 = u0 * gu, g1 = u1 * gu < groups ? u1 * gu : groups;
  b.x0 = nb == 1 ? 0 : g0 * 8;
  b.bw = nb == 1 ? c.nxh : (g1 - g0) * 8;
  return b;
}

// the workgroups of the row-based launches: dim3((unsigned)(8 * per_xcd * nxb))
static long long xcd_blocks(int nrows, int nxb, int rchunk) {
  const long long per_xcd = ((long long)nrows + 8LL * rchunk - 1) / (8LL * rchunk) * rchunk;
  return 8 * per_xcd * nxb;
}

// switch (c.p.n_lattices) { case 1: <1>; case 3: <3>; default: <4> }, then the four-way branch of every *_dispatch<NL>
struct Triple {
  int NL;
  bool PULL, EPHI;
};
template <int NL>
static Triple dispatch(bool streamed_state, bool ephi) {
  if (streamed_state) {
    if (ephi) return Triple{NL, false, (NL > 1)};
    else return Triple{NL, false, false};
  } else {
    if (ephi) return Triple{NL, true, (NL > 1)};
    else return Triple{NL, true, false};
  }
}
static Triple collide(int n_lattices, bool streamed_state, bool ephi) {
  switch (n_lattices) {
    case 1: return dispatch<1>(streamed_state, ephi);
    case 3: return dispatch<3>(streamed_state, ephi);
    default: return dispatch<4>(streamed_state, ephi);
  }
}

}  // namespace model

// ---- the sweep ---------------------------------------------------------------------------------------------------------------
static bool same(const ZPlan& p, const model::Launch& w) {
  return p.family == w.family && p.R == w.R && p.lanes == w.lanes && p.modes_per_wg == w.group && p.lds_bytes == w.lds && std::strcmp(p.name, w.name) == 0;
}
static ZPlan plan_of(const model::Ctx& c) {
  return z_solve_plan(c.slab ? c.slab_m : c.p.nz - 2, c.p.ny * c.nxh, c.nxh, c.tri_partition, c.tri_lds_ok, c.slab);
}

int main() {
  long cases = 0;
  std::vector<int> nys, nxhs;
  for (int i = 1; i <= 40; ++i) { nys.push_back(i); nxhs.push_back(i); }
  nys.push_back(512); nys.push_back(1024);
  nxhs.push_back(257); nxhs.push_back(513);

  // collide variant
  for (int nl : {1, 3, 4})
    for (int streamed = 0; streamed < 2; ++streamed)
      for (int ephi = 0; ephi < 2; ++ephi) {
        ++cases;
        const model::Triple w = model::collide(nl, streamed != 0, ephi != 0);
        const CollideVariant v = collide_variant(nl, streamed != 0, ephi != 0);
        CHECK(v.nl == w.NL && v.pull == w.PULL && v.ephi == w.EPHI, "collide variant of n_lattices %d streamed %d ephi %d: (%d, %d, %d)", nl, streamed, ephi, v.nl,
              (int)v.pull, (int)v.ephi);
        CHECK(nl > 1 || !v.ephi, "EPHI for one lattice");
      }

  // XCD grid
  for (int rchunk : {1, 8, 64})
    for (int nxb = 1; nxb <= 17; ++nxb)
      for (int nrows = 0; nrows <= 2100; ++nrows) {
        ++cases;
        CHECK(xcd_grid_blocks(nrows, nxb, rchunk) == model::xcd_blocks(nrows, nxb, rchunk), "grid of %d rows x %d blocks, runs of %d", nrows, nxb, rchunk);
      }
  CHECK(xcd_grid_blocks(1024 * 1026, 16, 64) == model::xcd_blocks(1024 * 1026, 16, 64), "grid of a 1024 x 1024 x 1026 lattice");

  // z-solve plan, whether it is a partition solve, and the column blocks of the single context's solve
  for (int slab = 0; slab < 2; ++slab)
    for (int tp = 0; tp <= 2; ++tp)
      for (int lds_ok = 0; lds_ok < 2; ++lds_ok)
        for (int ny : nys)
          for (int nxh : nxhs)
            for (int rows = 0; rows <= 600; ++rows) {
              ++cases;
              model::Ctx c{};
              c.p = model::Params{ny, rows + 2, 4};
              c.nxh = nxh; c.slab_m = rows; c.tri_partition = tp; c.tri_lds_ok = lds_ok != 0; c.slab = slab != 0; c.nranks = 2;
              const ZPlan p = plan_of(c);
              const model::Launch w = slab ? model::launch_slab_reduce_correct(c) : model::launch_tridiag(c);
              CHECK(same(p, w), "plan of rows %d ny %d nxh %d tri_partition %d lds %d slab %d: %s R %d lanes %d modes %d lds %d, model %s R %d lanes %d modes %d lds %d", rows,
                    ny, nxh, tp, lds_ok, slab, p.name, p.R, p.lanes, p.modes_per_wg, p.lds_bytes, w.name, w.R, w.lanes, w.group, w.lds);
              CHECK((p.row >= 0) == (p.family == ZFamily::partition), "table row %d of %s", p.row, p.name);
              if (p.row >= 0) CHECK(kZPartRows[p.row].R == p.R && kZPartRows[p.row].lanes == p.lanes && (slab || kZPartRows[p.row].single), "table row %d of %s", p.row, p.name);
              if (slab) {
                CHECK((p.family == ZFamily::partition) == model::stage1_is_slab_edges(c), "stage 1 of rows %d ny %d nxh %d tri_partition %d lds %d", rows, ny, nxh, tp, lds_ok);
                CHECK(!model::slab_read_once(c) || p.modes_per_wg == model::slab_part_modes(c), "slab_part_modes of rows %d ny %d nxh %d", rows, ny, nxh);
              } else {
                CHECK((p.family == ZFamily::partition) == model::tridiag_is_partition(c), "tridiag_is_partition of rows %d ny %d nxh %d tri_partition %d lds %d", rows, ny, nxh,
                      tp, lds_ok);
              }
              // poisson_blocks 0 .. 16 with and without the own transforms where the model lets blocks apply; elsewhere (a slab, no
              // partition solve: one block whatever else holds) the default and a request for three, own transforms present
              const bool may = !slab && model::tridiag_is_partition(c);
              for (int own = may ? 0 : 1; own < 2; ++own)
                for (int knob = 0; knob <= 16; ++knob) {
                  if (!may && knob != 0 && knob != 3) continue;
                  ++cases;
                  c.own_fft = own != 0;
                  c.poisson_blocks = knob;
                  const int nb = poisson_block_count(c.slab, c.own_fft, knob, p, nxh, ny, rows), wnb = model::poisson_block_count(c);
                  CHECK(nb == wnb, "poisson_block_count of rows %d ny %d nxh %d tri_partition %d lds %d slab %d own %d knob %d: %d, model %d", rows, ny, nxh, tp, lds_ok, slab,
                        own, knob, nb, wnb);
                  for (int k = 0; k < nb; ++k) {
                    const ColumnBlock b = column_block(nxh, ny, nb, k);
                    const model::ModeBlock wb = model::poisson_block(c, k);
                    CHECK(b.x0 == wb.x0 && b.bw == wb.bw, "poisson_block %d of %d, ny %d nxh %d: (%d, %d), model (%d, %d)", k, nb, ny, nxh, b.x0, b.bw, wb.x0, wb.bw);
                  }
                }
            }

  // the default of poisson_blocks (0): three blocks from 768 MiB of half spectrum on - beyond the sweep above, so here
  for (int ny : {512, 1024})
    for (int nxh : {264, 520})
      for (int rows = 60; rows <= 520; ++rows)
        for (int tp = 1; tp <= 2; ++tp) {
          ++cases;
          model::Ctx c{};
          c.p = model::Params{ny, rows + 2, 4};
          c.nxh = nxh; c.tri_partition = tp; c.tri_lds_ok = true; c.own_fft = true; c.poisson_blocks = 0;
          const ZPlan p = plan_of(c);
          CHECK(same(p, model::launch_tridiag(c)), "plan of rows %d ny %d nxh %d tri_partition %d", rows, ny, nxh, tp);
          const int nb = poisson_block_count(false, true, 0, p, nxh, ny, rows), wnb = model::poisson_block_count(c);
          CHECK(nb == wnb, "default poisson_block_count of rows %d ny %d nxh %d: %d, model %d", rows, ny, nxh, nb, wnb);
          for (int k = 0; k < nb; ++k) {
            const ColumnBlock b = column_block(nxh, ny, nb, k);
            const model::ModeBlock wb = model::poisson_block(c, k);
            CHECK(b.x0 == wb.x0 && b.bw == wb.bw, "default poisson_block %d of %d, ny %d nxh %d", k, nb, ny, nxh);
          }
        }

  // mode blocks of the slab solve: the knob 1 .. 16 (and 0, which means 1), every block below the count it comes to
  for (int ny : nys)
    for (int nxh : nxhs)
      for (int knob = 0; knob <= 16; ++knob) {
        model::Ctx c{};
        c.p = model::Params{ny, 102, 4};
        c.nxh = nxh; c.slab = true; c.slab_m = 100; c.nranks = 3; c.edge_chunks = knob;
        const int nb = edge_chunk_count(nxh, ny, knob), wnb = model::edge_chunk_count(c);
        CHECK(nb == wnb && nb >= 1, "edge_chunk_count of ny %d nxh %d knob %d: %d, model %d", ny, nxh, knob, nb, wnb);
        CHECK(block_unit_groups(nxh, ny) == model::block_unit_groups(c), "block_unit_groups of ny %d nxh %d", ny, nxh);
        int next = 0;
        for (int k = 0; k < nb; ++k) {
          ++cases;
          const ColumnBlock b = column_block(nxh, ny, nb, k);
          const model::ModeBlock wb = model::mode_block(c, k);
          CHECK(b.x0 == wb.x0 && b.bw == wb.bw, "mode_block %d of %d, ny %d nxh %d: (%d, %d), model (%d, %d)", k, nb, ny, nxh, b.x0, b.bw, wb.x0, wb.bw);
          if (nxh % 8 != 0) continue;
          // the blocks tile [0, nxh) in order, in whole 128-byte lines, in whole workgroups of whatever partition solve runs
          CHECK(b.x0 == next && b.bw > 0, "block %d of %d, ny %d nxh %d starts at %d, the one before ended at %d", k, nb, ny, nxh, b.x0, next);
          next = b.x0 + b.bw;
          CHECK(b.x0 % 8 == 0 && b.bw % 8 == 0, "block %d of %d, ny %d nxh %d: (%d, %d)", k, nb, ny, nxh, b.x0, b.bw);
          for (int slab = 0; slab < 2; ++slab)
            for (int rows : {1, 64, 65, 128, 129, 256, 257, 512}) {
              const ZPlan p = z_solve_plan(rows, ny * nxh, nxh, 2, true, slab != 0);
              if (p.family == ZFamily::partition)
                CHECK((ny * b.bw) % p.modes_per_wg == 0, "block %d of %d, ny %d nxh %d: %d modes, %s takes %d per workgroup", k, nb, ny, nxh, ny * b.bw, p.name, p.modes_per_wg);
            }
        }
        if (nxh % 8 == 0) CHECK(next == nxh, "blocks of ny %d nxh %d knob %d end at %d", ny, nxh, knob, next);
      }

  std::printf("ok %ld\n", cases);
  return 0;
}
