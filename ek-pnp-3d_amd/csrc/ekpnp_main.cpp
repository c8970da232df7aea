// ekpnp_main.cpp — thin C++ host over the C ABI that keeps main.cu's driver / IO surface.
//
// Same sequence as main.cu:19-296 of the reference: parameters -> banner -> (read previous data |
// initialization) -> init_equilibrium -> first Tecplot zone -> time loop {stream_collide_save;
// fast_Poisson; t += dt; every NSAVE steps a Tecplot zone; every printCurrent steps the wall
// current and a umax line} -> performance banner -> last zone -> data_end.dat.  Same file names
// (data.dat, umax.dat, data_end.dat), same cadence (i % NSAVE == 1, i % printCurrent == 1,
// main.cu:206,211), same text formats (the writers are in io.hip).
//
// What is different on purpose: the grid, the step count and the physics knobs are run-time
// options instead of compile-time constants (LBM.h:29-125); the "read previous data" question
// is a flag instead of scanf (main.cu:158-159); no system("pause") (main.cu:294); errors are
// reported and returned, not exit()ed from inside the library.  Only the C ABI of
// include/ekpnp.h is used: this file is also the worked example of INTEGRATION.md.
//
// --gpus N (N > 1) slab-decomposes the lattice along z over N GPUs of the node in THIS process
// (ekpnp_group_*: RCCL ring + all-gather over xGMI on a high-priority comm stream per GPU, halo
// exchange overlapped with the collision of the interior planes); same files, same formats.
// --devices 0,0,1,1 places the slabs by hand (slabs sharing a device exchange by device copies).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ekpnp.h"

// the lattice is either one context or a group of z slabs; the driver below does not care
static ekpnp_ctx* ctx = nullptr;
static ekpnp_group* grp = nullptr;

static bool group_path = false;  // --gpus N / --devices: errors live in the group's slot, also before the group exists

static int fail(const char* what, int rc) {
  std::fprintf(stderr, "ekpnp_main: %s failed (%d): %s\n", what, rc, group_path ? ekpnp_group_last_error(grp) : ekpnp_last_error(ctx));
  if (grp) ekpnp_group_destroy(grp);
  else if (ctx) ekpnp_destroy(ctx);
  return 1;
}
#define CK(call)                                   \
  do {                                             \
    int rc_ = (call);                              \
    if (rc_ != EKPNP_OK) return fail(#call, rc_);  \
  } while (0)
// one verb, two spellings
#define RUN(verb, ...) (grp ? ekpnp_group_##verb(grp, ##__VA_ARGS__) : ekpnp_##verb(ctx, ##__VA_ARGS__))

int main(int argc, char* argv[]) {
  // LBM.h:32-35,122-125
  int nx = 50, ny = 8, nz = 51;
  unsigned nsteps = 1000, nsave = 0, print_current = 50;
  int flag = 0;  // 1: read previous data (main.cu:161); 2: from the lossless data_end.bin
  int binary_state = 0;  // also write data_end.bin (ekpnp_save_state) at the end
  int lattices = 4;
  int gpus = 1, transport = EKPNP_TRANSPORT_AUTO;
  std::vector<int> devices;
  std::string out = ".";
  double exf = 0.0, uw = 0.0, chargeinf = -1.0, Ra = -1.0, TH = -1.0;
  double converged_tol = 0.0;  // > 0: ekpnp_initialization_converged instead of the reference's fixed 501 Picard sweeps
  unsigned profiles_every = 0;  // > 0: ekpnp_stats_accumulate after every that many iterations, profiles.dat at the end
  unsigned snap_every = 0;      // > 0: a coarsened FP32 snapshot snap_<step>.vtk after every that many iterations (ekpnp_snapshot_begin / _finish)
  ekpnp_snapshot_spec snap_spec = {0u, 1, 1, 1};
  unsigned monitor_every = 0;   // > 0: the scalar time series (ekpnp_monitor_*) with a row after every that many iterations, monitor.dat at the end
  ekpnp_monitor_spec mon_spec = {0u, 1, 1};
  // --seed-pattern: x-y structure added to the start fields on the device (ekpnp_seed), then fast_Poisson, then init_equilibrium
  bool seeding = false, seed_noise_given = false, seed_pattern_noise = false;
  ekpnp_seed_spec seed_spec = {(1u << EKPNP_C) | (1u << EKPNP_CN), EKPNP_SEED_NONE, 1, 1, 1, 0, 1u, 1.0e-3, 0.0};
  unsigned modes_every = 0;     // > 0: the energies of chosen x-y modes (ekpnp_modes_*) after every that many iterations, modes.dat at the end
  ekpnp_modes_spec modes_spec = {};
  modes_spec.field_id = EKPNP_UZ;
  modes_spec.nmodes = 0;        // 0: the seed's (mx, my), (mx, -my) and (0, 0)
  unsigned spectrum_every = 0;  // > 0: shells and peak of chosen planes' x-y power spectra (ekpnp_spectrum_*) after every that many iterations, spectrum.dat at the end
  ekpnp_spectrum_spec spectrum_spec = {};
  spectrum_spec.field_id = EKPNP_UZ;
  spectrum_spec.nplanes = 0;    // 0: the mid plane (nz - 1)/2
  unsigned hist_every = 0;      // > 0: a histogram (ekpnp_hist_*) of the planes --hist-planes names after every that many iterations, hist.dat at the end
  ekpnp_hist_spec hist_spec = {};
  hist_spec.a.value = EKPNP_HIST_Q;
  hist_spec.a.n = 128;
  hist_spec.b.value = EKPNP_UZ;
  hist_spec.b.n = 0;            // 0: no second axis
  bool hist_bins2_given = false, hist_axis2 = false;
  int hist_z_lo = -1, hist_z_hi = -1;  // -1: the interior planes 1 .. nz - 2
  unsigned section_every = 0;       // > 0: a section (ekpnp_section_arm / _record) of the planes --section-planes names after every that many iterations, section.dat at the end
  unsigned section_full_every = 0;  // > 0: a section of EVERY plane (ekpnp_section_save) after every that many iterations, section_<step>.dat each time
  ekpnp_section_spec section_spec = {};
  section_spec.values = (1u << EKPNP_SECTION_Q) | (1u << EKPNP_UZ);
  section_spec.across = EKPNP_ACROSS_Y;
  section_spec.lo = section_spec.hi = -1;  // -1: the whole axis
  // --tracers N / --tracers-grid: a particle cloud (ekpnp_tracers_*) advanced by h = M*dt after every M-th iteration (--tracers-every M), a row of
  // moments each time; tracers.dat and tracers_final.bin at the end, tracer_cells.dat with --tracers-cells
  bool tracers = false, tracers_box_given = false;
  ekpnp_tracers_spec tracers_spec = {};
  tracers_spec.mode = EKPNP_TRACERS_RANDOM;
  tracers_spec.seed = 1u;
  unsigned tracers_every = 1, tracers_sort_every = 0;  // --tracers-sort-every K: ekpnp_tracers_sort before every K-th advance (0: never)
  unsigned long long tracers_advances = 0;
  int tracers_substeps = 1, tracers_cells[3] = {0, 0, 0};
  double tracers_mu = 0.0;
  // --tracers-diffusivity D [--tracers-noise-seed S]: the advances are Brownian (ekpnp_tracers_advance_brownian)
  bool tracers_brownian = false, tracers_noise_seed_given = false;
  double tracers_D = 0.0;
  unsigned long long tracers_noise_seed = 0;
  // --tracers-absorb bottom|top|both [--arrivals-bins N] [--deposit-cells bx,by]: the advances are absorbing (ekpnp_tracers_advance_absorbing;
  // D from --tracers-diffusivity, else 0); landings.bin, arrivals.dat and deposit.dat at the end
  int tracers_absorb = 0, arrivals_bins = 0, deposit_cells[2] = {0, 0};
  // --tracers-stretch [--stretch-levels l_lo,n]: the advances carry the flow-map gradient (ekpnp_tracers_advance_tangent); stretch.bin and,
  // with --stretch-levels, stretch_levels.dat at the end
  bool tracers_stretch = false, stretch_levels_given = false;
  int stretch_levels[2] = {0, 0};
  // --tracks id,id,... / --tracks-first K: tagged particles of that cloud; after every M-th iteration (--tracks-every M, default --tracers-every) a row
  // of x, y, z, wx, wy and the --tracks-values of each goes to a ring (ekpnp_tracks_*); tracks.dat at the end
  bool tracks = false, tracks_flags = false;
  ekpnp_tracks_spec tracks_spec = {};
  unsigned tracks_every = 0;
  static const char* const field_names[EKPNP_NFIELDS] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"};
  auto field_id_of = [&](const char* q, size_t len) {
    for (int k = 0; k < EKPNP_NFIELDS; ++k)
      if (std::strlen(field_names[k]) == len && std::strncmp(field_names[k], q, len) == 0) return k;
    return -1;
  };
  auto value_id_of = [&](const char* q) { return std::strcmp(q, "q") == 0 ? (int)EKPNP_HIST_Q : field_id_of(q, std::strlen(q)); };
  int batch = 0;  // 1: ekpnp_step(n) from one output mark to the next instead of one stream_collide_save + fast_Poisson pair per iteration
  std::vector<std::pair<std::string, int>> tunes;  // --tune knob=value: ekpnp_tune / ekpnp_group_tune right after creation
  for (int i = 1; i < argc; ++i) {
    auto val = [&](const char* name) -> const char* {
      if (std::strcmp(argv[i], name) == 0 && i + 1 < argc) return argv[++i];
      return nullptr;
    };
    const char* v;
    if ((v = val("--nx"))) nx = std::atoi(v);
    else if ((v = val("--ny"))) ny = std::atoi(v);
    else if ((v = val("--nz"))) nz = std::atoi(v);
    else if ((v = val("--steps"))) nsteps = (unsigned)std::atoi(v);
    else if ((v = val("--nsave"))) nsave = (unsigned)std::atoi(v);
    else if ((v = val("--print-current"))) print_current = (unsigned)std::atoi(v);
    else if ((v = val("--read-previous"))) flag = std::atoi(v);
    else if ((v = val("--binary-state"))) binary_state = std::atoi(v);
    else if ((v = val("--lattices"))) lattices = std::atoi(v);
    else if ((v = val("--gpus"))) gpus = std::atoi(v);
    else if ((v = val("--transport"))) transport = !std::strcmp(v, "rccl") ? EKPNP_TRANSPORT_RCCL : !std::strcmp(v, "copy") ? EKPNP_TRANSPORT_COPY : EKPNP_TRANSPORT_AUTO;
    else if ((v = val("--devices"))) {
      devices.clear();
      for (const char* q = v; *q;) {
        devices.push_back(std::atoi(q));
        while (*q && *q != ',') ++q;
        if (*q == ',') ++q;
      }
    }
    else if ((v = val("--out"))) out = v;
    else if ((v = val("--exf"))) exf = std::atof(v);
    else if ((v = val("--uw"))) uw = std::atof(v);
    else if ((v = val("--chargeinf"))) chargeinf = std::atof(v);
    else if ((v = val("--Ra"))) Ra = std::atof(v);
    else if ((v = val("--TH"))) TH = std::atof(v);
    else if ((v = val("--converged-init"))) converged_tol = std::atof(v);
    else if ((v = val("--batch"))) batch = std::atoi(v);
    else if ((v = val("--profiles-every"))) profiles_every = (unsigned)std::atoi(v);
    else if ((v = val("--snap-every"))) snap_every = (unsigned)std::atoi(v);
    else if ((v = val("--snap-coarsen"))) {
      if (std::sscanf(v, "%d,%d,%d", &snap_spec.cx, &snap_spec.cy, &snap_spec.cz) != 3) { std::fprintf(stderr, "--snap-coarsen wants cx,cy,cz, got %s\n", v); return 2; }
    }
    else if ((v = val("--snap-fields"))) {
      static const char* const names[EKPNP_NFIELDS] = {"rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"};
      snap_spec.fields = 0u;
      for (const char* q = v; *q;) {
        const char* e = q;
        while (*e && *e != ',') ++e;
        int id = -1;
        for (int k = 0; k < EKPNP_NFIELDS; ++k)
          if (std::strlen(names[k]) == (size_t)(e - q) && std::strncmp(names[k], q, (size_t)(e - q)) == 0) id = k;
        if (id < 0) { std::fprintf(stderr, "--snap-fields wants names out of rho,c,cn,phi,ux,uy,uz,Ex,Ey,Ez,T, got %s\n", v); return 2; }
        snap_spec.fields |= 1u << id;
        q = *e ? e + 1 : e;
      }
    }
    else if ((v = val("--monitor-every"))) monitor_every = (unsigned)std::atoi(v);
    else if ((v = val("--monitor-quantities"))) {
      mon_spec.quantities = 0u;
      for (const char* q = v; *q;) {
        const char* e = q;
        while (*e && *e != ',') ++e;
        int id = -1;
        for (int k = 0; k < EKPNP_NMONITORS; ++k) {
          const char* name = ekpnp_monitor_name(k);
          if (std::strlen(name) == (size_t)(e - q) && std::strncmp(name, q, (size_t)(e - q)) == 0) id = k;
        }
        if (id < 0) {
          std::fprintf(stderr, "--monitor-quantities wants names out of");
          for (int k = 0; k < EKPNP_NMONITORS; ++k) std::fprintf(stderr, "%s%s", k ? "," : " ", ekpnp_monitor_name(k));
          std::fprintf(stderr, ", got %s\n", v);
          return 2;
        }
        mon_spec.quantities |= 1u << id;
        q = *e ? e + 1 : e;
      }
    }
    else if ((v = val("--seed-pattern"))) {
      seeding = true;
      seed_pattern_noise = false;
      if (!std::strcmp(v, "noise")) { seed_spec.pattern = EKPNP_SEED_NONE; seed_pattern_noise = true; }
      else if (!std::strcmp(v, "rolls")) seed_spec.pattern = EKPNP_SEED_ROLLS;
      else if (!std::strcmp(v, "squares")) seed_spec.pattern = EKPNP_SEED_SQUARES;
      else if (!std::strcmp(v, "hexagons")) seed_spec.pattern = EKPNP_SEED_HEXAGONS;
      else { std::fprintf(stderr, "--seed-pattern wants noise, rolls, squares or hexagons, got %s\n", v); return 2; }
    }
    else if ((v = val("--seed-modes"))) {
      if (std::sscanf(v, "%d,%d", &seed_spec.mx, &seed_spec.my) != 2) { std::fprintf(stderr, "--seed-modes wants mx,my, got %s\n", v); return 2; }
    }
    else if ((v = val("--seed-amplitude"))) seed_spec.amplitude = std::atof(v);
    else if ((v = val("--seed-noise"))) { seed_spec.noise = std::atof(v); seed_noise_given = true; }
    else if ((v = val("--seed-relative"))) seed_spec.relative = std::atoi(v);
    else if ((v = val("--seed"))) seed_spec.seed = std::strtoull(v, nullptr, 10);
    else if ((v = val("--seed-fields"))) {
      seed_spec.fields = 0u;
      for (const char* q = v; *q;) {
        const char* e = q;
        while (*e && *e != ',') ++e;
        const int id = field_id_of(q, (size_t)(e - q));
        if (id < 0) { std::fprintf(stderr, "--seed-fields wants names out of rho,c,cn,ux,uy,uz,T, got %.*s in %s\n", (int)(e - q), q, v); return 2; }
        seed_spec.fields |= 1u << id;
        q = *e ? e + 1 : e;
      }
    }
    else if ((v = val("--modes-every"))) modes_every = (unsigned)std::atoi(v);
    else if ((v = val("--modes-field"))) {
      const int id = field_id_of(v, std::strlen(v));
      if (id < 0) { std::fprintf(stderr, "--modes-field wants one of rho,c,cn,phi,ux,uy,uz,Ex,Ey,Ez,T, got %s\n", v); return 2; }
      modes_spec.field_id = id;
    }
    else if ((v = val("--modes"))) {
      modes_spec.nmodes = 0;
      for (const char* q = v; *q;) {
        int m = 0, n = 0, used = 0;
        if (std::sscanf(q, "%d,%d%n", &m, &n, &used) != 2 || modes_spec.nmodes >= EKPNP_MAX_MODES || (q[used] && q[used] != ';')) {
          std::fprintf(stderr, "--modes wants at most %d pairs \"m,n;m,n;...\", got %s\n", EKPNP_MAX_MODES, v);
          return 2;
        }
        modes_spec.m[modes_spec.nmodes] = m;
        modes_spec.n[modes_spec.nmodes] = n;
        ++modes_spec.nmodes;
        q += used;
        if (*q == ';') ++q;
      }
    }
    else if ((v = val("--spectrum-every"))) spectrum_every = (unsigned)std::atoi(v);
    else if ((v = val("--spectrum-field"))) {
      const int id = field_id_of(v, std::strlen(v));
      if (id < 0) { std::fprintf(stderr, "--spectrum-field wants one of rho,c,cn,phi,ux,uy,uz,Ex,Ey,Ez,T, got %s\n", v); return 2; }
      spectrum_spec.field_id = id;
    }
    else if ((v = val("--spectrum-planes"))) {
      spectrum_spec.nplanes = 0;
      for (const char* q = v; *q;) {
        int z = 0, used = 0;
        if (std::sscanf(q, "%d%n", &z, &used) != 1 || spectrum_spec.nplanes >= EKPNP_MAX_SPECTRUM_PLANES || (q[used] && q[used] != ',')) {
          std::fprintf(stderr, "--spectrum-planes wants at most %d plane indices \"z,z,...\", got %s\n", EKPNP_MAX_SPECTRUM_PLANES, v);
          return 2;
        }
        spectrum_spec.z[spectrum_spec.nplanes++] = z;
        q += used;
        if (*q == ',') ++q;
      }
    }
    else if ((v = val("--hist-every"))) hist_every = (unsigned)std::atoi(v);
    else if ((v = val("--hist-value")) || (v = val("--hist-value2"))) {
      const bool second = std::strcmp(argv[i - 1], "--hist-value2") == 0;
      const int id = value_id_of(v);
      if (id < 0) { std::fprintf(stderr, "%s wants one of rho,c,cn,phi,ux,uy,uz,Ex,Ey,Ez,T,q, got %s\n", argv[i - 1], v); return 2; }
      (second ? hist_spec.b : hist_spec.a).value = id;
      hist_axis2 = hist_axis2 || second;
    }
    else if ((v = val("--hist-bins"))) hist_spec.a.n = std::atoi(v);
    else if ((v = val("--hist-bins2"))) { hist_spec.b.n = std::atoi(v); hist_bins2_given = hist_axis2 = true; }
    else if ((v = val("--hist-range")) || (v = val("--hist-range2"))) {
      const bool second = std::strcmp(argv[i - 1], "--hist-range2") == 0;
      ekpnp_hist_axis& ax = second ? hist_spec.b : hist_spec.a;
      if (std::sscanf(v, "%lf,%lf", &ax.lo, &ax.hi) != 2) { std::fprintf(stderr, "%s wants lo,hi, got %s\n", argv[i - 1], v); return 2; }
      hist_axis2 = hist_axis2 || second;
    }
    else if ((v = val("--hist-planes"))) {
      if (std::sscanf(v, "%d,%d", &hist_z_lo, &hist_z_hi) != 2) { std::fprintf(stderr, "--hist-planes wants zlo,zhi, got %s\n", v); return 2; }
    }
    else if ((v = val("--section-every"))) section_every = (unsigned)std::atoi(v);
    else if ((v = val("--section-full-every"))) section_full_every = (unsigned)std::atoi(v);
    else if ((v = val("--section-values"))) {
      section_spec.values = 0u;
      for (const char* q = v; *q;) {
        const char* e = q;
        while (*e && *e != ',') ++e;
        const int id = (e - q == 1 && *q == 'q') ? (int)EKPNP_SECTION_Q : field_id_of(q, (size_t)(e - q));
        if (id < 0) { std::fprintf(stderr, "--section-values wants names out of rho,c,cn,phi,ux,uy,uz,Ex,Ey,Ez,T,q, got %.*s in %s\n", (int)(e - q), q, v); return 2; }
        section_spec.values |= 1u << id;
        q = *e ? e + 1 : e;
      }
    }
    else if ((v = val("--section-across"))) {
      if (!std::strcmp(v, "x")) section_spec.across = EKPNP_ACROSS_X;
      else if (!std::strcmp(v, "y")) section_spec.across = EKPNP_ACROSS_Y;
      else { std::fprintf(stderr, "--section-across wants x or y, got %s\n", v); return 2; }
    }
    else if ((v = val("--section-range"))) {
      if (std::sscanf(v, "%d,%d", &section_spec.lo, &section_spec.hi) != 2) { std::fprintf(stderr, "--section-range wants lo,hi, got %s\n", v); return 2; }
    }
    else if ((v = val("--section-planes"))) {
      section_spec.nplanes = 0;
      for (const char* q = v; *q;) {
        int z = 0, used = 0;
        if (std::sscanf(q, "%d%n", &z, &used) != 1 || section_spec.nplanes >= EKPNP_MAX_SECTION_PLANES || (q[used] && q[used] != ',')) {
          std::fprintf(stderr, "--section-planes wants at most %d plane indices \"z,z,...\", got %s\n", EKPNP_MAX_SECTION_PLANES, v);
          return 2;
        }
        section_spec.z[section_spec.nplanes++] = z;
        q += used;
        if (*q == ',') ++q;
      }
    }
    else if ((v = val("--tracers"))) {
      char* end = nullptr;
      const long long n = std::strtoll(v, &end, 10);
      if (end == v || *end) { std::fprintf(stderr, "--tracers wants a number of particles, got %s\n", v); return 2; }
      tracers = true;
      tracers_spec.mode = EKPNP_TRACERS_RANDOM;
      tracers_spec.n = n;
      tracers_spec.gx = tracers_spec.gy = tracers_spec.gz = 0;
    }
    else if ((v = val("--tracers-grid"))) {
      int used = 0;
      if (std::sscanf(v, "%d,%d,%d%n", &tracers_spec.gx, &tracers_spec.gy, &tracers_spec.gz, &used) != 3 || v[used]) { std::fprintf(stderr, "--tracers-grid wants gx,gy,gz, got %s\n", v); return 2; }
      tracers = true;
      tracers_spec.mode = EKPNP_TRACERS_GRID;
      tracers_spec.n = (int64_t)tracers_spec.gx * tracers_spec.gy * tracers_spec.gz;
    }
    else if ((v = val("--tracers-box"))) {
      int used = 0;
      if (std::sscanf(v, "%lf,%lf,%lf,%lf,%lf,%lf%n", &tracers_spec.lo[0], &tracers_spec.hi[0], &tracers_spec.lo[1], &tracers_spec.hi[1], &tracers_spec.lo[2], &tracers_spec.hi[2], &used) != 6 || v[used]) {
        std::fprintf(stderr, "--tracers-box wants x0,x1,y0,y1,z0,z1, got %s\n", v);
        return 2;
      }
      tracers_box_given = true;
    }
    else if ((v = val("--tracers-seed"))) {
      char* end = nullptr;
      tracers_spec.seed = std::strtoull(v, &end, 10);
      if (end == v || *end) { std::fprintf(stderr, "--tracers-seed wants a number, got %s\n", v); return 2; }
    }
    else if ((v = val("--tracers-every"))) {
      const int m = std::atoi(v);
      if (m < 1) { std::fprintf(stderr, "--tracers-every wants a number of iterations >= 1, got %s\n", v); return 2; }
      tracers_every = (unsigned)m;
    }
    else if ((v = val("--tracers-sort-every"))) {
      const int k = std::atoi(v);
      if (k < 1) { std::fprintf(stderr, "--tracers-sort-every wants a number of advances >= 1, got %s\n", v); return 2; }
      tracers_sort_every = (unsigned)k;
    }
    else if ((v = val("--tracers-substeps"))) {
      tracers_substeps = std::atoi(v);
      if (tracers_substeps < 1 || tracers_substeps > 4096) { std::fprintf(stderr, "--tracers-substeps wants 1 .. 4096, got %s\n", v); return 2; }
    }
    else if ((v = val("--tracers-mobility"))) {
      char* end = nullptr;
      tracers_mu = std::strtod(v, &end);
      if (end == v || *end) { std::fprintf(stderr, "--tracers-mobility wants a number (m^2/V/s), got %s\n", v); return 2; }
    }
    else if ((v = val("--tracers-diffusivity"))) {
      char* end = nullptr;
      tracers_D = std::strtod(v, &end);
      if (end == v || *end) { std::fprintf(stderr, "--tracers-diffusivity wants a number (m^2/s), got %s\n", v); return 2; }
      tracers_brownian = true;
    }
    else if ((v = val("--tracers-noise-seed"))) {
      char* end = nullptr;
      tracers_noise_seed = std::strtoull(v, &end, 10);
      if (end == v || *end) { std::fprintf(stderr, "--tracers-noise-seed wants a number, got %s\n", v); return 2; }
      tracers_noise_seed_given = true;
    }
    else if ((v = val("--tracers-absorb"))) {
      tracers_absorb = !std::strcmp(v, "bottom") ? 1 : !std::strcmp(v, "top") ? 2 : !std::strcmp(v, "both") ? 3 : 0;
      if (!tracers_absorb) { std::fprintf(stderr, "--tracers-absorb wants bottom, top or both, got %s\n", v); return 2; }
    }
    else if (std::strcmp(argv[i], "--tracers-stretch") == 0) tracers_stretch = true;  // (a flag: it takes no value)
    else if ((v = val("--stretch-levels"))) {
      int used = 0;
      if (std::sscanf(v, "%d,%d%n", &stretch_levels[0], &stretch_levels[1], &used) != 2 || v[used]) { std::fprintf(stderr, "--stretch-levels wants l_lo,n, got %s\n", v); return 2; }
      if (stretch_levels[1] < 1 || stretch_levels[1] > 4096) { std::fprintf(stderr, "--stretch-levels wants 1 .. 4096 levels, got %s\n", v); return 2; }
      stretch_levels_given = true;
    }
    else if ((v = val("--arrivals-bins"))) {
      arrivals_bins = std::atoi(v);
      if (arrivals_bins < 1 || arrivals_bins > 4096) { std::fprintf(stderr, "--arrivals-bins wants 1 .. 4096, got %s\n", v); return 2; }
    }
    else if ((v = val("--deposit-cells"))) {
      int used = 0;
      if (std::sscanf(v, "%d,%d%n", &deposit_cells[0], &deposit_cells[1], &used) != 2 || v[used]) { std::fprintf(stderr, "--deposit-cells wants bx,by, got %s\n", v); return 2; }
    }
    else if ((v = val("--tracers-cells"))) {
      int used = 0;
      if (std::sscanf(v, "%d,%d,%d%n", &tracers_cells[0], &tracers_cells[1], &tracers_cells[2], &used) != 3 || v[used]) { std::fprintf(stderr, "--tracers-cells wants bx,by,bz, got %s\n", v); return 2; }
    }
    else if ((v = val("--tracks"))) {
      tracks = tracks_flags = true;
      tracks_spec.ntags = 0;
      for (const char* q = v; *q;) {
        char* end = nullptr;
        const long id = std::strtol(q, &end, 10);
        if (end == q || (*end && *end != ',') || id < -2147483647L || id > 2147483647L) { std::fprintf(stderr, "--tracks wants id,id,..., got %s\n", v); return 2; }
        if (tracks_spec.ntags == EKPNP_TRACERS_MAX_TRACKS) { std::fprintf(stderr, "--tracks wants at most %d ids, got %s\n", EKPNP_TRACERS_MAX_TRACKS, v); return 2; }
        tracks_spec.ids[tracks_spec.ntags++] = (int32_t)id;
        q = *end ? end + 1 : end;
      }
    }
    else if ((v = val("--tracks-first"))) {
      const int k = std::atoi(v);
      if (k < 1 || k > EKPNP_TRACERS_MAX_TRACKS) { std::fprintf(stderr, "--tracks-first wants 1 .. %d, got %s\n", EKPNP_TRACERS_MAX_TRACKS, v); return 2; }
      tracks = tracks_flags = true;
      tracks_spec.ntags = k;
      for (int q = 0; q < k; ++q) tracks_spec.ids[q] = q;
    }
    else if ((v = val("--tracks-values"))) {
      tracks_flags = true;
      tracks_spec.nvalues = 0;
      for (const char* q = v; *q;) {
        const char* e = q;
        while (*e && *e != ',') ++e;
        const int id = (e - q == 1 && *q == 'q') ? (int)EKPNP_TRACERS_Q : field_id_of(q, (size_t)(e - q));
        if (id < 0 || tracks_spec.nvalues == EKPNP_TRACERS_MAX_VALUES) { std::fprintf(stderr, "--tracks-values wants at most 12 names out of rho,c,cn,phi,ux,uy,uz,Ex,Ey,Ez,T,q, got %.*s in %s\n", (int)(e - q), q, v); return 2; }
        tracks_spec.values[tracks_spec.nvalues++] = id;
        q = *e ? e + 1 : e;
      }
    }
    else if ((v = val("--tracks-every"))) {
      const int m = std::atoi(v);
      if (m < 1) { std::fprintf(stderr, "--tracks-every wants a number of iterations >= 1, got %s\n", v); return 2; }
      tracks_flags = true;
      tracks_every = (unsigned)m;
    }
    else if ((v = val("--tune"))) {
      const char* eq = std::strchr(v, '=');
      if (!eq || eq == v) { std::fprintf(stderr, "--tune wants knob=value, got %s\n", v); return 2; }
      tunes.emplace_back(std::string(v, eq), std::atoi(eq + 1));
    }
    else {
      std::fprintf(stderr,
                   "usage: ekpnp_main [--nx N --ny N --nz N] [--steps N] [--nsave N] [--print-current N] [--read-previous 0|1|2]\n"
                   "                  [--binary-state 0|1] [--gpus N [--transport auto|rccl|copy] [--devices d0,d1,...]]\n"
                   "                  [--lattices 1|3|4] [--exf F --uw U --chargeinf C --Ra R --TH T] [--out DIR] [--converged-init TOL]\n"
                   "                  [--tune knob=value ...] [--batch 0|1] [--profiles-every N]\n"
                   "                  [--snap-every N [--snap-coarsen cx,cy,cz] [--snap-fields rho,uz,...]]\n"
                   "                  [--monitor-every N [--monitor-quantities current_top,uz_max,...]]\n"
                   "                  [--seed-pattern noise|rolls|squares|hexagons [--seed-modes mx,my] [--seed-amplitude A] [--seed-noise B]\n"
                   "                   [--seed-fields c,cn,...] [--seed-relative 0|1] [--seed N]]\n"
                   "                  [--modes-every N [--modes-field uz] [--modes \"m,n;m,n;...\"]]\n"
                   "                  [--spectrum-every N [--spectrum-field uz] [--spectrum-planes z,z,...]]\n"
                   "                  [--hist-every N --hist-value q --hist-bins 128 --hist-range lo,hi\n"
                   "                   [--hist-value2 uz --hist-bins2 64 --hist-range2 lo,hi] [--hist-planes zlo,zhi]]\n"
                   "                  [--section-every N | --section-full-every N  [--section-values q,uz] [--section-across y]\n"
                   "                   [--section-range lo,hi] [--section-planes z,z,...]]\n"
                   "                  [--tracers N | --tracers-grid gx,gy,gz  [--tracers-box x0,x1,y0,y1,z0,z1] [--tracers-seed S] [--tracers-every M]\n"
                   "                   [--tracers-substeps k] [--tracers-mobility mu] [--tracers-cells bx,by,bz] [--tracers-sort-every K]\n"
                   "                   [--tracers-diffusivity D [--tracers-noise-seed S]]\n"
                   "                   [--tracers-absorb bottom|top|both [--arrivals-bins N] [--deposit-cells bx,by]]\n"
                   "                   [--tracers-stretch [--stretch-levels l_lo,n]]\n"
                   "                   [--tracks id,id,... | --tracks-first K  [--tracks-values T,q,...] [--tracks-every M]]]\n"
                   "  --tracers N: N particles at random places (--tracers-seed S, default 1) - or --tracers-grid gx,gy,gz: the centres of a\n"
                   "  gx x gy x gz grid - of the box --tracers-box (lattice units; default the interior 0,nx,0,ny,1,nz-2) are advected on the\n"
                   "  device (ekpnp_tracers_*, a single GPU only): after every M-th iteration (--tracers-every, default 1) the cloud moves by\n"
                   "  h = M*dt through the fields of that moment, in k midpoint substeps (--tracers-substeps, default 1), with the velocity\n"
                   "  u + mu E (--tracers-mobility, m^2/V/s; default 0: a passive tracer), and a row of moments - alive, lost, the sums of the\n"
                   "  unwrapped displacements and of their squares, of z and z^2, min and max z - is appended to a ring in device memory\n"
                   "  (enqueued only, nothing waits).  tracers.dat (ekpnp_tracers_ring_save) and tracers_final.bin (ekpnp_tracers_save) are written\n"
                   "  at the end, and with --tracers-cells bx,by,bz the final counts per cell as text, tracer_cells.dat.  Advancing every M\n"
                   "  iterations uses the fields at the end of the interval: exact in a steady flow, first order in M*dt otherwise.  With\n"
                   "  --batch 1 the batches are cut at these marks; both loops write the same bytes, and every other file is unchanged.\n"
                   "  --tracers-sort-every K (K >= 1; default: never): before every K-th advance the cloud is sorted into memory order on the\n"
                   "  device (ekpnp_tracers_sort), which keeps a stirred cloud's advance at the cost of an ordered one; no trajectory changes,\n"
                   "  the sums of tracers.dat may differ in their last bits, and tracers_final.bin then carries the particles' ids after wy.\n"
                   "  --tracers-diffusivity D (m^2/s, >= 0; default: none, a deterministic cloud): every substep also kicks each particle by a\n"
                   "  uniform increment of variance 2 D h per axis and reflects it at the plates (ekpnp_tracers_advance_brownian); the numbers\n"
                   "  are those of (--tracers-noise-seed S, default 0; the particle's id; the substep's number), so a sort changes no path and\n"
                   "  both loops write the same bytes; tracers_final.bin then carries the number of Brownian substeps taken.\n"
                   "  --tracers-absorb bottom|top|both: those plates keep what reaches them (ekpnp_tracers_advance_absorbing; D from\n"
                   "  --tracers-diffusivity, else 0: drift alone deposits) and every particle's first arrival is recorded on the device.  At\n"
                   "  the end landings.bin (ekpnp_landings_save), arrivals.dat - per wall the histogram of the arrival epochs 0 .. final in\n"
                   "  --arrivals-bins N cells (default 16) - and deposit.dat - both plates' maps in --deposit-cells bx,by cells (default 8,8,\n"
                   "  clipped to the lattice) - are written; the same bytes from both loops.\n"
                   "  --tracers-stretch (a flag; not with --tracers-diffusivity or --tracers-absorb): the advances also carry every particle's\n"
                   "  flow-map gradient F * 2^e along (ekpnp_tracers_stretch_begin after the seed, ekpnp_tracers_advance_tangent for every\n"
                   "  advance; the positions are those of the plain advance, bit for bit).  At the end stretch.bin (ekpnp_tracers_stretch_save) is\n"
                   "  written, and with --stretch-levels l_lo,n (1 <= n <= 4096) stretch_levels.dat: the particles without a level and the n + 2\n"
                   "  counts of floor(log2 |F 2^e|^2) below l_lo, at l_lo .. l_lo + n - 1 and above; the same bytes from both loops.\n"
                   "  --tracks id,id,... (at most 1024 particle ids of that cloud, the index a particle has when it is seeded) or --tracks-first K\n"
                   "  (ids 0 .. K-1): after every M-th iteration (--tracks-every, default --tracers-every), after that iteration's advance, a row\n"
                   "  of x, y, z, the image counts and the --tracks-values (names out of the fields and q = c - cn, interpolated at the particle\n"
                   "  as the advance does; default none) of each tagged particle is appended to a ring in device memory (ekpnp_tracks_arm /\n"
                   "  ekpnp_tracks_record: enqueued only, nothing waits); tracks.dat is written at the end (ekpnp_tracks_save: one line per row\n"
                   "  and tag).  With --batch 1 the batches are cut at these marks; both loops write the same bytes.\n"
                   "  --seed-pattern P: after the start-up (or the restart read) a pattern with mx,my whole periods across nx and ny (default 1,1)\n"
                   "  and amplitude A (default 1e-3) plus white noise of amplitude B (default 0; reproducible from --seed N, default 1) is added to\n"
                   "  the fields --seed-fields names (default c,cn; out of rho,c,cn,ux,uy,uz,T) on the interior planes, under a sin(pi z/(nz-1))\n"
                   "  envelope, relative to the field's value (--seed-relative 1, the default: v += v*s) or absolute (0: v += s) - on the device\n"
                   "  (ekpnp_seed: no field crosses the bus); then ekpnp_fast_poisson, then the usual init_equilibrium.  P = noise: no pattern,\n"
                   "  B defaults to 1e-3.  A seed with A = B = 0 changes nothing and is skipped together with its solve: every file is then byte\n"
                   "  for byte what it is without the flag.\n"
                   "  --modes-every N: after every N-th iteration the field --modes-field names (default uz) is projected onto the x-y modes of\n"
                   "  --modes (default: the seed's mx,my; mx,-my; and 0,0) on the device, and the energies E = sum_z |coefficient|^2 are appended\n"
                   "  to a ring in device memory (ekpnp_modes_arm / ekpnp_modes_record: enqueued only, nothing waits); modes.dat is written at the\n"
                   "  end (ekpnp_modes_save: one row per sample, %%.17g).  With --batch 1 the batches are cut at these marks; both loops write the\n"
                   "  same bytes, and every other file is unchanged.\n"
                   "  --spectrum-every N: after every N-th iteration the x-y power spectrum of the field --spectrum-field names (default uz) on\n"
                   "  the planes --spectrum-planes names (at most 16 global z, ascending; default the mid plane (nz-1)/2) is taken on the device:\n"
                   "  the shell spectrum E(k) and the dominant mode of each plane are appended to a ring in device memory (ekpnp_spectrum_arm /\n"
                   "  ekpnp_spectrum_record: enqueued only, nothing waits); spectrum.dat is written at the end (ekpnp_spectrum_save: one row per\n"
                   "  sample and plane, %%.17g).  With --batch 1 the batches are cut at these marks; both loops write the same bytes, and every\n"
                   "  other file is unchanged.\n"
                   "  --section-every N: after every N-th iteration the --section-values (names out of the fields and q = c - cn; default q,uz)\n"
                   "  summed along --section-across (x keeps y, y keeps x; default y) over the index range --section-range lo,hi (inclusive;\n"
                   "  default the whole axis, lo = hi: a cut) on the planes --section-planes (global z, ascending, at most 16; default the mid\n"
                   "  plane) are appended to a ring in device memory (ekpnp_section_arm / ekpnp_section_record: enqueued only, nothing waits);\n"
                   "  section.dat is written at the end (ekpnp_section_ring_save: one row per sample, value and plane).  --section-full-every N:\n"
                   "  the same values, axis and range on EVERY plane, written at once to section_<step>.dat (ekpnp_section_save; --section-planes\n"
                   "  does not apply).  With --batch 1 the batches are cut at these marks; both loops write the same bytes, and every other file\n"
                   "  is unchanged.\n"
                   "  --hist-every N: after every N-th iteration the histogram of --hist-value (a field or q = c - cn; default q) with --hist-bins\n"
                   "  bins (default 128) between --hist-range lo,hi - or, with any of --hist-value2 / --hist-bins2 (default 64) / --hist-range2, its\n"
                   "  joint histogram with that second value - summed over the planes --hist-planes zlo,zhi (global z, inclusive; default the\n"
                   "  interior 1,nz-2) is counted on the device and appended to a ring in device memory (ekpnp_hist_arm / ekpnp_hist_record:\n"
                   "  enqueued only, nothing waits); hist.dat is written at the end (ekpnp_hist_save: one row of integer counts per sample, under-\n"
                   "  and overflow cells included).  With --batch 1 the batches are cut at these marks; both loops write the same bytes, and every\n"
                   "  other file is unchanged.\n"
                   "  --monitor-every N: after every N-th iteration eleven scalars - the current through either plate, the wall gradients of\n"
                   "  T, max uz, the sums of u.u, c - cn, (c - cn)^2 and uz*T, max |rho - rho0| and the number of non-finite nodes - are reduced\n"
                   "  on the device and appended to a ring in device memory (ekpnp_monitor_arm / ekpnp_monitor_record: enqueued only, nothing\n"
                   "  waits); monitor.dat is written at the end (ekpnp_monitor_save: one row per sample, %%.17g).  With --batch 1 the batches\n"
                   "  are NOT cut at these marks: the rows are appended from inside ekpnp_step.  Both loops write the same bytes, and every\n"
                   "  other file is unchanged.  --monitor-quantities: only those columns (the others hold 0 and cost nothing).\n"
                   "  --snap-every N: after every N-th iteration a coarsened FP32 snapshot of the fields goes to snap_<step, 7 digits>.vtk (legacy\n"
                   "  VTK, big-endian floats: ParaView and VisIt read it as is).  z is sampled every cz-th plane (cz divides nz - 1: both plates are\n"
                   "  kept), x and y are means over cx x cy blocks (each 1, 2, 4 or 8); default 1,1,1 and all eleven fields.  The snapshot is\n"
                   "  begun at the mark (ekpnp_snapshot_begin: coarsened on the device, copied out on a side stream) and its file is written at\n"
                   "  the next mark or at the end (ekpnp_snapshot_finish), while the time loop runs on; every other file is unchanged.\n"
                   "  --profiles-every N: after every N-th iteration the plane sums of the fields (z profiles of the fields, their squares,\n"
                   "  the fluxes uz*T, uz*c, uz*cn and the body force (c - cn)*E; reduced on the device, ekpnp_stats_accumulate) are added to\n"
                   "  running sums, and the time-averaged plane means go to profiles.dat at the end (ekpnp_save_profiles); every other file is\n"
                   "  byte for byte what it is without the flag.\n"
                   "  --batch 1: the time loop advances with ONE ekpnp_step(ctx, n) call from each output mark (Tecplot zone, current / umax\n"
                   "  line) to the next, with the knob batch_moments on (only the last step of a call stores rho, u, c, cn, T: nothing looks at\n"
                   "  the steps in between); the same files, byte for byte, as the default loop, which mirrors main.cu:189-224 call by call.\n"
                   "  --tune knob=value: a launch-shape or transport knob of include/ekpnp.h's ekpnp_tune (with --gpus N: on every slab), e.g.\n"
                   "  edge_chunks=4 (the slab Poisson solve's all-gather in 4 pipelined blocks), lead_planes=0, inline_exchanges=0, comm_cus=8;\n"
                   "  the results are the same bits under every setting.\n"
                   "  --converged-init TOL: Poisson-Boltzmann start-up with a convergence test and a damping that cannot diverge\n"
                   "  (ekpnp_initialization_converged); the reference's 501 sweeps with PB_omega = 0.05 (LBM.cu:89-106) diverge to NaN on\n"
                   "  channels taller than about 180 planes at the default spacing.\n"
                   "  --read-previous 1: restart from data_end.dat (%%10.6f text, the reference's); 2: from data_end.bin (--binary-state 1,\n"
                   "  the 11 fields as raw FP64).  Both restarts are the reference's (main.cu:161-175): the populations are rebuilt as the\n"
                   "  EQUILIBRIUM of the fields, so a restarted run is not the bitwise continuation of the interrupted one.\n");
      return 2;
    }
  }
  if (seeding) {
    if (seed_pattern_noise) {  // noise alone: A = 0, B from --seed-noise
      seed_spec.amplitude = 0.0;
      if (!seed_noise_given) seed_spec.noise = 1.0e-3;
    }
  }
  if (modes_every && modes_spec.nmodes == 0) {  // the seed's mode, its mirror image in y and the plane mean
    const int mx = seed_spec.mx, my = seed_spec.my;
    auto fold = [&](int n) { return ny % 2 == 0 && n == -(ny / 2) ? ny / 2 : n; };  // -ny/2 is the Nyquist mode ny/2
    const int cand[3][2] = {{mx, fold(my)}, {mx, fold(-my)}, {0, 0}};
    for (const auto& mn : cand) {
      bool dup = false;
      for (int j = 0; j < modes_spec.nmodes; ++j) dup = dup || (modes_spec.m[j] == mn[0] && modes_spec.n[j] == mn[1]);
      if (dup) continue;
      modes_spec.m[modes_spec.nmodes] = mn[0];
      modes_spec.n[modes_spec.nmodes] = mn[1];
      ++modes_spec.nmodes;
    }
  }
  if (spectrum_every && spectrum_spec.nplanes == 0) {
    spectrum_spec.nplanes = 1;
    spectrum_spec.z[0] = (nz - 1) / 2;
  }
  if (hist_every) {
    if (hist_axis2 && !hist_bins2_given) hist_spec.b.n = 64;
    if (hist_z_lo < 0 && hist_z_hi < 0) { hist_z_lo = nz > 2 ? 1 : 0; hist_z_hi = nz > 2 ? nz - 2 : nz - 1; }
  }
  ekpnp_section_spec section_full_spec = section_spec;
  if (section_every || section_full_every) {
    if (section_spec.lo < 0 && section_spec.hi < 0) { section_spec.lo = 0; section_spec.hi = (section_spec.across == EKPNP_ACROSS_X ? nx : ny) - 1; }
    section_full_spec = section_spec;
    section_full_spec.nplanes = 0;
    if (section_spec.nplanes == 0) {
      section_spec.nplanes = 1;
      section_spec.z[0] = (nz - 1) / 2;
    }
  }
  if (tracers && !tracers_box_given) {  // the interior
    tracers_spec.lo[0] = 0.0; tracers_spec.hi[0] = (double)nx;
    tracers_spec.lo[1] = 0.0; tracers_spec.hi[1] = (double)ny;
    tracers_spec.lo[2] = 1.0; tracers_spec.hi[2] = (double)(nz - 2);
  }
  if (nsave == 0) nsave = nsteps / 2 ? nsteps / 2 : 1;  // LBM.h:123
  if (print_current == 0) print_current = 1;

  if (!devices.empty()) gpus = (int)devices.size();
  if (gpus < 1) gpus = 1;
  ekpnp_params P;
  if (ekpnp_default_params(&P, nx, ny, nz) != EKPNP_OK) return fail("ekpnp_default_params", 1);
  if (nx == 50 && ny == 8 && nz == 51) { P.Lx = 0.5e-6; P.Ly = 0.08e-6; P.Lz = 0.5e-6; }  // literals of LBM.h:40-42
  P.n_lattices = lattices;
  P.exf = exf; P.uw = uw;  // main.cu:30-31
  if (chargeinf >= 0.0) P.chargeinf = chargeinf;
  if (Ra >= 0.0) P.Ra = Ra;
  if (TH >= 0.0) P.TH = TH;

  if (seeding && ekpnp_seed_spec_check(&P, &seed_spec) != EKPNP_OK) { std::fprintf(stderr, "ekpnp_main: --seed-*: %s\n", ekpnp_last_error(nullptr)); return 2; }
  if (modes_every && ekpnp_modes_spec_check(&P, &modes_spec) != EKPNP_OK) { std::fprintf(stderr, "ekpnp_main: --modes*: %s\n", ekpnp_last_error(nullptr)); return 2; }

  if (spectrum_every && ekpnp_spectrum_spec_check(&P, &spectrum_spec) != EKPNP_OK) { std::fprintf(stderr, "ekpnp_main: --spectrum*: %s\n", ekpnp_last_error(nullptr)); return 2; }
  if (hist_every && (ekpnp_hist_spec_check(&P, &hist_spec) != EKPNP_OK ||
                     ekpnp_hist_range_check(&P, hist_z_lo, hist_z_hi, (int)((nsteps + hist_every - 1) / hist_every ? (nsteps + hist_every - 1) / hist_every : 1)) != EKPNP_OK)) {
    std::fprintf(stderr, "ekpnp_main: --hist*: %s\n", ekpnp_last_error(nullptr));
    return 2;
  }
  if ((section_every && ekpnp_section_spec_check(&P, &section_spec) != EKPNP_OK) || (section_full_every && ekpnp_section_spec_check(&P, &section_full_spec) != EKPNP_OK)) {
    std::fprintf(stderr, "ekpnp_main: --section*: %s\n", ekpnp_last_error(nullptr));
    return 2;
  }
  if (tracers_sort_every && !tracers) { std::fprintf(stderr, "ekpnp_main: --tracers-sort-every %u: there is no cloud to sort (give --tracers N or --tracers-grid gx,gy,gz)\n", tracers_sort_every); return 2; }
  if ((tracers_brownian || tracers_noise_seed_given) && !tracers) { std::fprintf(stderr, "ekpnp_main: --tracers-diffusivity / --tracers-noise-seed: there is no cloud to diffuse (give --tracers N or --tracers-grid gx,gy,gz)\n"); return 2; }
  if (tracers_noise_seed_given && !tracers_brownian) { std::fprintf(stderr, "ekpnp_main: --tracers-noise-seed %llu: there is no noise to seed (give --tracers-diffusivity D)\n", tracers_noise_seed); return 2; }
  if (tracers_brownian && (!std::isfinite(tracers_D) || tracers_D < 0.0)) { std::fprintf(stderr, "ekpnp_main: --tracers-diffusivity: tracers: D = %.17g (must be finite and >= 0)\n", tracers_D); return 2; }
  if ((arrivals_bins || deposit_cells[0]) && !tracers_absorb) { std::fprintf(stderr, "ekpnp_main: --arrivals-bins / --deposit-cells: no plate absorbs (give --tracers-absorb bottom|top|both)\n"); return 2; }
  if (stretch_levels_given && !tracers_stretch) { std::fprintf(stderr, "ekpnp_main: --stretch-levels: nothing is stretched (give --tracers-stretch)\n"); return 2; }
  if (tracers_stretch) {
    if (!tracers) { std::fprintf(stderr, "ekpnp_main: --tracers-stretch: there is no cloud to stretch (give --tracers N or --tracers-grid gx,gy,gz)\n"); return 2; }
    if (tracers_brownian || tracers_absorb) { std::fprintf(stderr, "ekpnp_main: --tracers-stretch goes with the deterministic advance only, not with --tracers-diffusivity or --tracers-absorb\n"); return 2; }
  }
  if (tracers_absorb) {
    if (!tracers) { std::fprintf(stderr, "ekpnp_main: --tracers-absorb: there is no cloud to deposit (give --tracers N or --tracers-grid gx,gy,gz)\n"); return 2; }
    if (!arrivals_bins) arrivals_bins = 16;
    if (!deposit_cells[0]) { deposit_cells[0] = nx < 8 ? nx : 8; deposit_cells[1] = ny < 8 ? ny : 8; }
    if (ekpnp_tracers_cell(&P, deposit_cells[0], deposit_cells[1], 1, 0.0, 0.0, 0.0) < -1) { std::fprintf(stderr, "ekpnp_main: --deposit-cells: %s\n", ekpnp_last_error(nullptr)); return 2; }
  }
  if (tracks_flags) {
    if (gpus > 1 || !devices.empty()) { std::fprintf(stderr, "ekpnp_main: --tracks*: tracers: slab contexts are not supported (one GPU only)\n"); return 2; }
    if (!tracers) { std::fprintf(stderr, "ekpnp_main: --tracks*: there is no cloud to tag (give --tracers N or --tracers-grid gx,gy,gz)\n"); return 2; }
    if (!tracks) { std::fprintf(stderr, "ekpnp_main: --tracks-values / --tracks-every: no particle is tagged (give --tracks id,id,... or --tracks-first K)\n"); return 2; }
    if (!tracks_every) tracks_every = tracers_every;
    if (ekpnp_tracks_spec_check(&P, tracers_spec.n, &tracks_spec) != EKPNP_OK) { std::fprintf(stderr, "ekpnp_main: --tracks*: %s\n", ekpnp_last_error(nullptr)); return 2; }
  }
  if (tracers) {
    if (gpus > 1 || !devices.empty()) { std::fprintf(stderr, "ekpnp_main: --tracers*: tracers: slab contexts are not supported (one GPU only)\n"); return 2; }
    if (ekpnp_tracers_spec_check(&P, &tracers_spec) != EKPNP_OK) { std::fprintf(stderr, "ekpnp_main: --tracers*: %s\n", ekpnp_last_error(nullptr)); return 2; }
    if (tracers_cells[0] && ekpnp_tracers_cell(&P, tracers_cells[0], tracers_cells[1], tracers_cells[2], 0.0, 0.0, 0.0) < -1) {
      std::fprintf(stderr, "ekpnp_main: --tracers-cells: %s\n", ekpnp_last_error(nullptr));
      return 2;
    }
  }

  // main.cu:40-52
  std::printf("Simulating 3D electrokinetic flow with heat transfer vortices\n");
  std::printf("      domain size (NX x NY x NZ): %ux%ux%u\n", (unsigned)nx, (unsigned)ny, (unsigned)nz);
  std::printf("               Ra: %g\n", P.Ra);
  std::printf("               Pr: %g\n", P.nu / P.D);  // compute_parameters, LBM.cu:2445
  std::printf("            uwall: %g\n", P.uw);
  std::printf("   External force: %g\n", P.exf);
  std::printf("        timesteps: %u\n", nsteps);
  std::printf("       save every: %u\n", nsave);
  std::printf("    message every: %u\n", nsave);
  std::printf("\n");

  if (gpus > 1 || !devices.empty()) {
    group_path = true;
    int rc = ekpnp_group_create(&P, gpus, devices.empty() ? nullptr : devices.data(), transport, &grp);
    if (rc != EKPNP_OK) return fail("ekpnp_group_create", rc);
  } else {
    int rc = ekpnp_create(&P, &ctx);
    if (rc != EKPNP_OK) return fail("ekpnp_create", rc);
  }
  if (batch) tunes.insert(tunes.begin(), std::make_pair(std::string("batch_moments"), 1));  // (an explicit --tune batch_moments=0 comes later and wins)
  for (const auto& kv : tunes) {
    const int rc = grp ? ekpnp_group_tune(grp, kv.first.c_str(), kv.second) : ekpnp_tune(ctx, kv.first.c_str(), kv.second);
    if (rc != EKPNP_OK) return fail(("--tune " + kv.first).c_str(), rc);
  }
  std::printf("HIP information\n");
  if (grp)
    std::printf("      z slabs: %d, halo transport: %s\n", ekpnp_group_size(grp), ekpnp_group_transport(grp) == EKPNP_TRANSPORT_RCCL ? "RCCL" : "device copies");
  std::printf("      device memory held by the solver: %.1f MiB\n\n", (double)(grp ? ekpnp_group_device_bytes(grp) : ekpnp_device_bytes(ctx)) / (1024.0 * 1024.0));

  const std::string f_data = out + "/data.dat", f_umax = out + "/umax.dat", f_end = out + "/data_end.dat";
  const std::string f_bin = out + "/data_end.bin";
  double t = 0.0;
  if (flag == 1) {  // main.cu:161-164
    std::printf("Reading previous data...\n");
    CK(RUN(read_data, f_end.c_str(), &t));
  } else if (flag == 2) {  // the same restart from the lossless file
    std::printf("Reading previous data (binary)...\n");
    CK(RUN(read_state, f_bin.c_str(), &t));
  } else {  // main.cu:165-171
    std::printf("Initializing...\n");
    if (converged_tol > 0.0) {
      int sweeps = 0;
      double res = 0.0;
      CK(RUN(initialization_converged, converged_tol, 200000, &sweeps, &res));
      std::printf("      Poisson-Boltzmann start-up: %d sweeps, relative residual %.2e\n", sweeps, res);
    } else {
      CK(RUN(initialization));
    }
    t = 0.0;
  }
  CK(RUN(set_time, t));
  if (seeding && (seed_spec.amplitude != 0.0 || seed_spec.noise != 0.0)) {  // (A = B = 0 adds nothing: the fields and phi stay what the start-up left)
    CK(RUN(seed, &seed_spec));     // enqueues only: the pass runs on the device, no field moves
    CK(RUN(fast_poisson));         // phi and E of the seeded c, cn
  }
  CK(RUN(init_equilibrium));                             // main.cu:174
  CK(RUN(save_data_tecplot, f_data.c_str(), 0, t, 1));   // main.cu:178-179 ("wb+")
  { FILE* f = std::fopen(f_umax.c_str(), "wb"); if (f) std::fclose(f); }  // main.cu:180

  if (monitor_every) {  // a ring that holds the whole run
    mon_spec.every = (int32_t)monitor_every;
    mon_spec.capacity = (int32_t)((nsteps + monitor_every - 1) / monitor_every);
    if (mon_spec.capacity < 1) mon_spec.capacity = 1;
    CK(RUN(monitor_arm, &mon_spec));
  }
  if (modes_every) CK(RUN(modes_arm, &modes_spec, (int)((nsteps + modes_every - 1) / modes_every ? (nsteps + modes_every - 1) / modes_every : 1)));  // a ring that holds the whole run
  if (spectrum_every) CK(RUN(spectrum_arm, &spectrum_spec, (int)((nsteps + spectrum_every - 1) / spectrum_every ? (nsteps + spectrum_every - 1) / spectrum_every : 1)));  // a ring that holds the whole run
  if (hist_every) CK(RUN(hist_arm, &hist_spec, hist_z_lo, hist_z_hi, (int)((nsteps + hist_every - 1) / hist_every ? (nsteps + hist_every - 1) / hist_every : 1)));  // a ring that holds the whole run
  if (section_every) CK(RUN(section_arm, &section_spec, (int)((nsteps + section_every - 1) / section_every ? (nsteps + section_every - 1) / section_every : 1)));  // a ring that holds the whole run
  if (tracers) {  // the cloud at its start positions and a ring that holds the whole run
    CK(ekpnp_tracers_seed(ctx, &tracers_spec));
    if (tracers_stretch) CK(ekpnp_tracers_stretch_begin(ctx));
    CK(ekpnp_tracers_arm(ctx, (int)(nsteps / tracers_every ? nsteps / tracers_every : 1)));
    if (tracks) CK(ekpnp_tracks_arm(ctx, &tracks_spec, (int)(nsteps / tracks_every ? nsteps / tracks_every : 1)));
  }
  CK(RUN(synchronize));
  const auto begin = std::chrono::steady_clock::now();  // main.cu:185-186
  for (unsigned i = 0; i < nsteps; i++) {               // main.cu:189-224
    if (batch) {
      // iterations i .. j in one call, j = the next iteration something looks at the fields (or the last one)
      unsigned j = i;
      while (j + 1 < nsteps && !(j % nsave == 1 || j % print_current == 1 || (profiles_every && (j + 1) % profiles_every == 0) ||
                                 (snap_every && (j + 1) % snap_every == 0) || (modes_every && (j + 1) % modes_every == 0) ||
                                 (spectrum_every && (j + 1) % spectrum_every == 0) || (hist_every && (j + 1) % hist_every == 0) ||
                                 (section_every && (j + 1) % section_every == 0) || (section_full_every && (j + 1) % section_full_every == 0) ||
                                 (tracers && (j + 1) % tracers_every == 0) || (tracks && (j + 1) % tracks_every == 0))) ++j;
      CK(RUN(step, (int)(j - i + 1)));
      for (unsigned k = i; k <= j; ++k) t = t + P.dt;  // the same additions as the loop below makes, so the files carry the same time
      i = j;
    } else {
      CK(RUN(stream_collide_save, t));
      CK(RUN(fast_poisson));
      t = t + P.dt;
    }
    if (i % nsave == 1) {
      CK(RUN(save_data_tecplot, f_data.c_str(), 1, t, 1));
      std::printf("Iteration: %u, physical time: %g.\n", i, t);
    }
    if (i % print_current == 1) {
      double I = 0.0;
      CK(RUN(current, &I));  // reduced on the device (main.cu:212-215 copies 3 fields to the host)
      std::printf("Iteration: %u, physical time: %g, Current = %g\n", i, t, I);
      CK(RUN(record_umax, f_umax.c_str(), 1, t));
    }
    if (monitor_every && !batch && (i + 1) % monitor_every == 0) CK(RUN(monitor_record, (int64_t)(i + 1), t));  // enqueues only (--batch 1: ekpnp_step has done it)
    if (modes_every && (i + 1) % modes_every == 0) CK(RUN(modes_record, (int64_t)(i + 1), t));  // enqueues only
    if (spectrum_every && (i + 1) % spectrum_every == 0) CK(RUN(spectrum_record, (int64_t)(i + 1), t));  // enqueues only
    if (hist_every && (i + 1) % hist_every == 0) CK(RUN(hist_record, (int64_t)(i + 1), t));  // enqueues only
    if (section_every && (i + 1) % section_every == 0) CK(RUN(section_record, (int64_t)(i + 1), t));  // enqueues only
    if (section_full_every && (i + 1) % section_full_every == 0) {
      char name[40];
      std::snprintf(name, sizeof name, "/section_%07u.dat", i + 1);
      CK(RUN(section_save, &section_full_spec, (out + name).c_str(), t));  // waits for this one map: [values][nz][nkeep] doubles
    }
    if (tracers && (i + 1) % tracers_every == 0) {  // enqueues only: the cloud moves through the fields of this moment
      if (tracers_sort_every && ++tracers_advances % tracers_sort_every == 0) CK(ekpnp_tracers_sort(ctx));
      if (tracers_absorb) CK(ekpnp_tracers_advance_absorbing(ctx, tracers_mu, tracers_D, (double)tracers_every * P.dt, tracers_substeps, (uint64_t)tracers_noise_seed, tracers_absorb));
      else if (tracers_brownian) CK(ekpnp_tracers_advance_brownian(ctx, tracers_mu, tracers_D, (double)tracers_every * P.dt, tracers_substeps, (uint64_t)tracers_noise_seed));
      else if (tracers_stretch) CK(ekpnp_tracers_advance_tangent(ctx, tracers_mu, (double)tracers_every * P.dt, tracers_substeps));
      else CK(ekpnp_tracers_advance(ctx, tracers_mu, (double)tracers_every * P.dt, tracers_substeps));
      CK(ekpnp_tracers_record(ctx, (int64_t)(i + 1), t));
    }
    if (tracks && (i + 1) % tracks_every == 0) CK(ekpnp_tracks_record(ctx, (int64_t)(i + 1), t));  // enqueues only: after this iteration's advance
    if (profiles_every && (i + 1) % profiles_every == 0) CK(RUN(stats_accumulate));  // enqueues only: the loop runs on
    if (snap_every && (i + 1) % snap_every == 0) {
      char name[32];
      std::snprintf(name, sizeof name, "/snap_%07u.vtk", i + 1);
      CK(RUN(snapshot_finish));  // the file of the previous mark: its copy landed long ago, the device keeps stepping meanwhile
      CK(RUN(snapshot_begin, &snap_spec, (out + name).c_str(), t));  // enqueues only
    }
  }
  if (snap_every) CK(RUN(snapshot_finish));
  CK(RUN(synchronize));
  const double runtime = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();

  // main.cu:241-251
  const double nodes_updated = (double)nsteps * (double)nx * (double)ny * (double)nz;
  std::printf(" ----- performance information -----\n");
  std::printf("               timesteps: %u\n", nsteps);
  std::printf("           clock runtime: %.3f (s)\n", runtime);
  std::printf("                   speed: %.2f (Mlups)\n", nodes_updated / (1e6 * runtime));

  CK(RUN(save_data_tecplot, f_data.c_str(), 1, t, 1));  // main.cu:253
  CK(RUN(save_data_end, f_end.c_str(), 0, t));          // main.cu:256-257
  if (binary_state) CK(RUN(save_state, f_bin.c_str(), t));
  if (profiles_every) CK(RUN(save_profiles, (out + "/profiles.dat").c_str(), t));
  if (monitor_every) CK(RUN(monitor_save, (out + "/monitor.dat").c_str()));
  if (modes_every) CK(RUN(modes_save, (out + "/modes.dat").c_str()));
  if (spectrum_every) CK(RUN(spectrum_save, (out + "/spectrum.dat").c_str()));
  if (hist_every) CK(RUN(hist_save, (out + "/hist.dat").c_str()));
  if (section_every) CK(RUN(section_ring_save, (out + "/section.dat").c_str()));
  if (tracers) {
    CK(ekpnp_tracers_ring_save(ctx, (out + "/tracers.dat").c_str()));
    CK(ekpnp_tracers_save(ctx, (out + "/tracers_final.bin").c_str(), t));
    if (tracks) CK(ekpnp_tracks_save(ctx, (out + "/tracks.dat").c_str()));
    if (tracers_absorb) {
      int64_t final_epoch = 0;
      CK(ekpnp_tracers_epoch(ctx, &final_epoch));
      if (final_epoch == 0) CK(ekpnp_tracers_advance_absorbing(ctx, 0.0, 0.0, 0.0, 1, 0, tracers_absorb));  // (no advance fell into the run: a step of no length makes the record)
      CK(ekpnp_landings_save(ctx, (out + "/landings.bin").c_str()));
      CK(ekpnp_tracers_epoch(ctx, &final_epoch));
      const int64_t width = final_epoch / arrivals_bins + 1;  // cells 1 .. N cover the epochs 0 .. final
      FILE* f = std::fopen((out + "/arrivals.dat").c_str(), "wb");
      if (!f) { std::fprintf(stderr, "ekpnp_main: cannot open arrivals.dat\n"); ekpnp_destroy(ctx); return 1; }
      std::fprintf(f, "# ekpnp arrivals nx %d ny %d nz %d n %lld epoch %lld e0 0 width %lld nbins %d: per wall (1 bottom, 2 top) the wall, none, and the nbins + 2 counts\n", nx, ny, nz,
                   (long long)tracers_spec.n, (long long)final_epoch, (long long)width, arrivals_bins);
      std::vector<int64_t> counts((size_t)arrivals_bins + 2);
      for (int wall = 1; wall <= 2; ++wall) {
        int64_t none = 0;
        CK(ekpnp_landings_hist(ctx, wall, 0, width, arrivals_bins, counts.data(), &none));
        std::fprintf(f, "%d %lld", wall, (long long)none);
        for (int64_t v : counts) std::fprintf(f, " %lld", (long long)v);
        std::fprintf(f, "\n");
      }
      std::fclose(f);
      const int bx = deposit_cells[0], by = deposit_cells[1];
      f = std::fopen((out + "/deposit.dat").c_str(), "wb");
      if (!f) { std::fprintf(stderr, "ekpnp_main: cannot open deposit.dat\n"); ekpnp_destroy(ctx); return 1; }
      std::fprintf(f, "# ekpnp deposit nx %d ny %d nz %d bx %d by %d n %lld epoch %lld: per wall (1 bottom, 2 top) a line `wall elsewhere`, then by rows of bx counts\n", nx, ny, nz, bx, by,
                   (long long)tracers_spec.n, (long long)final_epoch);
      counts.assign((size_t)bx * by, 0);
      for (int wall = 1; wall <= 2; ++wall) {
        int64_t elsewhere = 0;
        CK(ekpnp_landings_map(ctx, wall, bx, by, 0, final_epoch, counts.data(), &elsewhere));
        std::fprintf(f, "%d %lld\n", wall, (long long)elsewhere);
        for (int r = 0; r < by; ++r) {
          for (int k = 0; k < bx; ++k) std::fprintf(f, "%s%lld", k ? " " : "", (long long)counts[(size_t)r * bx + k]);
          std::fprintf(f, "\n");
        }
      }
      std::fclose(f);
    }
    if (tracers_stretch) {
      CK(ekpnp_tracers_stretch_save(ctx, (out + "/stretch.bin").c_str()));
      if (stretch_levels_given) {
        const int l_lo = stretch_levels[0], nlevels = stretch_levels[1];
        std::vector<int64_t> counts((size_t)nlevels + 2);
        int64_t none = 0;
        CK(ekpnp_tracers_stretch_levels(ctx, l_lo, nlevels, counts.data(), &none));
        FILE* f = std::fopen((out + "/stretch_levels.dat").c_str(), "wb");
        if (!f) { std::fprintf(stderr, "ekpnp_main: cannot open stretch_levels.dat\n"); ekpnp_destroy(ctx); return 1; }
        std::fprintf(f, "# ekpnp stretch levels nx %d ny %d nz %d n %lld l_lo %d nlevels %d time %.17g: none, then the nlevels + 2 counts (below, l_lo .., at or above l_lo + nlevels)\n",
                     nx, ny, nz, (long long)tracers_spec.n, l_lo, nlevels, t);
        std::fprintf(f, "%lld", (long long)none);
        for (int64_t v : counts) std::fprintf(f, " %lld", (long long)v);
        std::fprintf(f, "\n");
        std::fclose(f);
      }
    }
    if (tracers_cells[0]) {
      const int bx = tracers_cells[0], by = tracers_cells[1], bz = tracers_cells[2];
      std::vector<int64_t> counts((size_t)bx * by * bz);
      int64_t lost = 0;
      CK(ekpnp_tracers_cell_counts(ctx, bx, by, bz, counts.data(), &lost));
      FILE* f = std::fopen((out + "/tracer_cells.dat").c_str(), "wb");
      if (!f) { std::fprintf(stderr, "ekpnp_main: cannot open tracer_cells.dat\n"); ekpnp_destroy(ctx); return 1; }
      std::fprintf(f, "# ekpnp tracer cells nx %d ny %d nz %d bx %d by %d bz %d n %lld lost %lld time %.17g\n", nx, ny, nz, bx, by, bz, (long long)tracers_spec.n, (long long)lost, t);
      for (int r = 0; r < by * bz; ++r) {  // one row per (cz, cy), cx along the row
        for (int k = 0; k < bx; ++k) std::fprintf(f, "%s%lld", k ? " " : "", (long long)counts[(size_t)r * bx + k]);
        std::fprintf(f, "\n");
      }
      std::fclose(f);
    }
  }
  CK(grp ? ekpnp_group_destroy(grp) : ekpnp_destroy(ctx));    // main.cu:264-290
  return 0;
}
