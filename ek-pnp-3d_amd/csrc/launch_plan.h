// launch_plan.h — which kernel instantiation runs, and on which grid: every such decision of the hot path, once.
// Pure functions of plain integers and bools: no HIP, includable by a plain C++ compiler (tests/plan_check.cpp compares them with
// the predicates they replaced).  The launchers (lbm_kernels.hip, poisson.hip) ask here and turn the answer into a launch; bits
// depend on the answers - a mode must be eliminated by the same instantiation wherever it is solved - so nothing else decides.
#pragma once
#include <cstddef>
#include <type_traits>
#include <utility>

namespace ekpnp {

// ---- collide sweep: (NL, PULL, EPHI) of k_collide_* ------------------------------------------------------------------------
// NL lattices (1, 3, anything else: 4), PULL unless the state is kept streamed, EPHI (E formed from phi inside the collide)
// only where there is a lattice that drifts in E: never for NL = 1.
struct CollideVariant {
  int nl;
  bool pull, ephi;
};
constexpr CollideVariant collide_variant(int n_lattices, bool streamed_state, bool takes_e_from_phi) {
  const int nl = n_lattices == 1 ? 1 : n_lattices == 3 ? 3 : 4;
  return CollideVariant{nl, !streamed_state, nl > 1 && takes_e_from_phi};
}

// ---- XCD-aware grids: rows dealt to the 8 XCDs in runs of `rchunk` -----------------------------------------------------------
// rows per XCD rounded up to whole runs - the 8 XCDs together cover [0, 8 per_xcd) >= nrows -, nxb workgroups per row
constexpr long long xcd_grid_blocks(int nrows, int nxb, int rchunk) {
  const long long per_xcd = ((long long)nrows + 8LL * rchunk - 1) / (8LL * rchunk) * rchunk;
  return 8 * per_xcd * nxb;
}

// ---- z solve -----------------------------------------------------------------------------------------------------------------
// The partition solves (k_tridiag_part<R, LANES> of a single context, k_slab_part<R, LANES> of a slab): LANES lanes of a wavefront
// hold R rows each of one mode, a workgroup of 8 wavefronts takes 8 * 64 / LANES adjacent modes and R x 8 KB of LDS.  The first row
// of this table whose conditions hold is the instantiation: columns of up to `max_rows` unknown rows, a whole spectrum of a
// multiple of `mode_multiple` modes (short columns share a wavefront where that leaves whole workgroups).  A single context has no
// <2,64>: its columns of 65 .. 128 rows go on to <8,32> or <4>.
struct ZPartRow {
  int max_rows, mode_multiple, R, lanes;
  bool single;  // also an instantiation of k_tridiag_part (every row is one of k_slab_part)
  const char* single_name;
  const char* slab_name;
};
constexpr ZPartRow kZPartRows[] = {
    {128, 32, 8, 16, true, "k_tridiag_part<8,16>", "k_slab_part<8,16>"},
    {128, 1, 2, 64, false, nullptr, "k_slab_part<2>"},
    {256, 16, 8, 32, true, "k_tridiag_part<8,32>", "k_slab_part<8,32>"},
    {256, 1, 4, 64, true, "k_tridiag_part<4>", "k_slab_part<4>"},
    {512, 1, 8, 64, true, "k_tridiag_part<8>", "k_slab_part<8>"},
};
constexpr int kZPartRowCount = (int)(sizeof(kZPartRows) / sizeof(kZPartRows[0]));
// f(std::integral_constant<int, i>) for every row i of the table (the launchers instantiate the kernels from it)
template <class F, std::size_t... I>
constexpr void for_each_zpart_row(F&& f, std::index_sequence<I...>) {
  (f(std::integral_constant<int, (int)I>{}), ...);
}
template <class F>
constexpr void for_each_zpart_row(F&& f) {
  for_each_zpart_row(f, std::make_index_sequence<kZPartRowCount>{});
}

enum class ZFamily {
  pcr64,        // k_tridiag_pcr64: one wavefront per mode, a row per lane
  serial,       // k_tridiag: one thread per mode
  partition,    // k_tridiag_part<R, LANES>; on a slab k_slab_edges, then k_slab_part<R, LANES>
  slab_serial,  // k_slab_thomas_local, then k_slab_reduce_correct: one thread per mode
};
struct ZPlan {
  ZFamily family;
  int row;           // of kZPartRows (partition), else -1
  int R, lanes;      // rows per lane, lanes per mode (serial kernels: the whole column in 1 lane, R = 0)
  int modes_per_wg;  // the grid is the launch's modes over this: exactly (partition) or rounded up
  int lds_bytes;     // dynamic LDS
  const char* name;  // what note_launch is told (slab families: the second kernel of the pair)
};
// rows: unknown rows of the column (NZ - 2, or the slab's own); nm = ny nxh: modes of the WHOLE spectrum, never of a block;
// tri_partition: 0 the serial sweeps everywhere (the A/B partner), 1 the partition solve on large lattices, 2 wherever it
// applies; tri_lds_ok: the device grants the dynamic LDS.
constexpr ZPlan z_solve_plan(int rows, int nm, int nxh, int tri_partition, bool tri_lds_ok, bool slab) {
  const bool part = tri_partition > 0 && tri_lds_ok && nxh % 8 == 0;
  bool wanted = false;
  if (slab) {
    wanted = part && rows >= 1 && rows <= 512;
  } else {
    if (rows <= 64) return ZPlan{ZFamily::pcr64, -1, 1, 64, 4, 0, "k_tridiag_pcr64"};  // whatever the knob says
    // enough modes to fill the chip 8 at a time
    const bool large = tri_partition > 1 || (std::size_t)nm * (std::size_t)rows >= (std::size_t)4 * 1024 * 1024;
    wanted = part && large;
  }
  if (wanted)
    for (int i = 0; i < kZPartRowCount; ++i) {
      const ZPartRow& r = kZPartRows[i];
      if ((slab || r.single) && rows <= r.max_rows && nm % r.mode_multiple == 0)
        return ZPlan{ZFamily::partition, i, r.R, r.lanes, 8 * (64 / r.lanes), r.R * 8192, slab ? r.slab_name : r.single_name};
    }
  if (slab) return ZPlan{ZFamily::slab_serial, -1, 0, 1, 64, 0, "k_slab_reduce_correct"};
  return ZPlan{ZFamily::serial, -1, 0, 1, 64, 0, "k_tridiag"};
}

// ---- kx column blocks of the half spectrum -------------------------------------------------------------------------------------
// The nxh / 8 column groups (8 kx columns = one 128-byte line of every row) are dealt to the blocks as evenly as they go, in
// units of `gu` groups such that every block holds whole workgroups of any partition instantiation (ny 8 gu a multiple of 32
// modes; gu = 1 wherever ny is a multiple of 4).  The units depend on the lattice only: the same on every rank of a slab team.
constexpr int gcd_int(int a, int b) { return b == 0 ? a : gcd_int(b, a % b); }
constexpr int block_unit_groups(int nxh, int ny) { return nxh % 8 != 0 ? 1 : 4 / gcd_int(4, ny); }
constexpr int block_unit_count(int nxh, int ny) {
  const int gu = block_unit_groups(nxh, ny);
  return (nxh / 8 + gu - 1) / gu;
}
struct ColumnBlock {
  int x0, bw;  // kx in [x0, x0 + bw)
};
// block k of nblocks (a count that edge_chunk_count / poisson_block_count returned); one block is the whole spectrum
constexpr ColumnBlock column_block(int nxh, int ny, int nblocks, int k) {
  if (nxh % 8 != 0 || nblocks == 1) return ColumnBlock{0, nxh};
  const int groups = nxh / 8, gu = block_unit_groups(nxh, ny), units = block_unit_count(nxh, ny);
  const int u0 = (int)((long long)units * k / nblocks), u1 = (int)((long long)units * (k + 1) / nblocks);
  const int g0 = u0 * gu, g1 = u1 * gu < groups ? u1 * gu : groups;
  return ColumnBlock{g0 * 8, (g1 - g0) * 8};
}
// mode blocks of a slab's z solve: the knob Ctx::edge_chunks, at most one block per unit
constexpr int edge_chunk_count(int nxh, int ny, int edge_chunks) {
  if (nxh % 8 != 0) return 1;
  const int units = block_unit_count(nxh, ny);
  return edge_chunks < 1 ? 1 : (edge_chunks > units ? units : edge_chunks);
}
// column blocks of a single context's solve: only where the library's own column passes and a partition solve run; the knob
// Ctx::poisson_blocks, or (0) three blocks from 768 MiB of half spectrum (16-byte modes) on, one below
constexpr int poisson_block_count(bool slab, bool own_fft, int poisson_blocks, const ZPlan& plan, int nxh, int ny, int rows) {
  if (slab || !own_fft || poisson_blocks == 1 || plan.family != ZFamily::partition) return 1;
  int want = poisson_blocks;
  if (want <= 0) want = (std::size_t)ny * nxh * (std::size_t)rows * 16 >= ((std::size_t)768 << 20) ? 3 : 1;
  const int units = block_unit_count(nxh, ny);
  return want > units ? units : want;
}

}  // namespace ekpnp
