// examples/driver.cpp -- a small C++ host driver over the plug-in surface, mirroring the call sequence of the
// reference's standalone/mmf_simplified/driver.cpp (:120-191 set-up, :237-272 time loop) for the dycore alone:
//
//   coupler.allocate_coupler_state -> set_grid -> [micro.init: tracer registration + constants] -> dycore.init
//   -> (host model fills the coupler fields) -> dycore.declare_current_profile_as_hydrostatic
//   -> N x { coupler.run_module("dycore", dycore.timeStep); [sponge_layer]; [micro.timeStep] } -> output
//
//   driver [--gpus N] [--tile R] [--bench K W] [--accelerate A [--accel-uv] [--accel-max-ttend X]] [--vt RATE [--vt-u] [--vt-limit L]]
//          <input.bin> <output.bin>
//
// --gpus N: the ensemble is sharded by member index over N devices of this node -- ONE host thread, ONE coupler and ONE dycore
// handle per device (hipSetDevice before init), no inter-device halo and no collective library: the exchanges the reference
// semantics need are the two sub-cycling steps, each a minimum over ALL members -- the dynamics time step (awfl/Dycore.h:86-101,
// 141-145) and, with the Kessler microphysics, its sedimentation step (kessler/Microphysics.h:385-390) -- taken here over N host
// doubles behind a barrier (HostMin) and handed to Dycore::timeStep(coupler, dt_dyn) / Microphysics::timeStep(coupler, rainsplit).  With fewer devices than ranks the ranks share
// devices (rehearsal on a 1-GPU box; bit-identical results, tests/test_cpp_driver.py).
// --tile R: the input's members are repeated R times along nens (tile t gets +t mK on temp so that no two CRMs are equal).
// --accelerate A: CRM mean-state acceleration (modules/mean_state_acceleration.h): the file's nsteps are the CRM steps of ONE GCM step,
// run on modules::MsaClock; the cease flag is global over the members, so the ranks OR theirs on the host through the same HostMin
// (the maximum of 0 / 1 is minus the minimum of their negatives).  Rank 0 prints the number of CRM steps that ran.
// --hyperdiff TAU: horizontal hyperdiffusion (modules/hyperdiffusion.h) with the time scale TAU (seconds) every CRM step after the sponge layer.
// --vt RATE: CRM variance transport (modules/variance_transport.h): the file's nsteps are the CRM steps of ONE GCM step; there is no GCM
// here, so the variance tendency is RATE (a relative growth rate per second) times the variance the step starts from.  Everything is
// per member: no exchange between the ranks.
// --bench K W: W untimed + K timed steps between barriers; rank 0 prints one JSON line with the wall time (bench.py --launcher cpp).
//
// Input/output are raw little-endian fp64 files written/read by tests/test_cpp_driver.py (the reference reads YAML and
// writes netCDF; neither library exists in this image and I/O is out of scope):
//   header (8 x int64): nens nx ny nz num_tracers nsteps flags has_consts ; then xlen ylen crm_dt (3 x f64),
//   (flags: bit0 = hydrostasis mode A, bit1 = run modules::sponge_layer, bit2 = Kessler Microphysics: its init registers
//   the three water tracers, so num_tracers must be 3, and "precl" (ny*nx*nens) is appended to the output)
//   6 constants (R_d cp_d R_v cp_v p0 grav), zint (nz+1), tracer flags (num_tracers x 2 bytes positive/adds_mass,
//   then idWV int64), then density_dry,uvel,vvel,wvel,temp,(tracers...) each nz*ny*nx*nens f64.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <thread>

// The dycore is selected by the include path, as in PAM (dynamics/CMakeLists.txt:5-17: -DPAM_DYCORE=<dir> puts
// dynamics/<dir> first): -Ipam_amd/csrc/host/dynamics/awfl_amd for the MI355X AWFL step, .../dynamics/spam_surface for
// the SPAM-surface stub of BASELINE config C5 (built with -DPAMC_DYCORE, like the reference's SPAM builds).
#include "Dycore.h"
#include "modules/gcm_forcing.h"     // compiled here; exercised from Python (tests/test_modules.py)
#include "modules/sponge_layer.h"
#include "modules/broadcast_initial_gcm_column.h"
#include "modules/perturb_temperature.h"
#include "modules/saturation_adjustment.h"
#include "modules/surface_friction.h"
#include "modules/surface_fluxes.h"
#include "modules/large_scale_forcing.h"
#include "modules/scalar_momentum.h"
#include "modules/horizontal_average.h"
#include "modules/time_average.h"
#include "modules/mean_state_acceleration.h"
#include "modules/variance_transport.h"
#include "modules/hyperdiffusion.h"
#include "modules/radiation_aggregate.h"
#include "modules/crm_feedback.h"
#include "modules/column_diagnostics.h"
#include "modules/flux_profiles.h"
#include "vertical_interp.h"
#include "physics/micro/kessler_amd/Microphysics.h"
#define PAM_MICRO_CLASS MicrophysicsIce   // the driver holds both Microphysics classes and picks at run time (--micro-ice)
#include "physics/micro/ice_amd/Microphysics.h"
#undef PAM_MICRO_CLASS
#include "physics/sgs/none/SGS.h"
#define PAM_SGS_CLASS SGSSmagorinsky      // the driver holds both SGS classes and picks at run time (--sgs-smag)
#include "physics/sgs/smag_amd/SGS.h"
#undef PAM_SGS_CLASS
#define PAM_SGS_CLASS SGSTke              // the third: the prognostic-TKE closure (--sgs-tke)
#include "physics/sgs/tke_amd/SGS.h"
#undef PAM_SGS_CLASS
#include "physics/radiation/forced_amd/radiation.h"
#define PAM_RAD_CLASS RadiationGray     // the driver holds both Radiation classes and picks at run time (--radiation-gray)
#include "physics/radiation/gray_amd/radiation.h"
#undef PAM_RAD_CLASS

#include <map>
#include <sstream>

static void die(const char *m) { std::fprintf(stderr, "driver: %s\n", m); std::exit(2); }

// min over the ranks' values: N host doubles behind a barrier.  A rank that fails releases the others (they throw too).
class HostMin {
  std::mutex m;
  std::condition_variable cv;
  const int n;
  int arrived = 0;
  long gen = 0;
  bool failed = false;
  std::vector<double> v;
  double result = 0;
 public:
  explicit HostMin(int n_) : n(n_), v(n_, 0.0) {}
  double operator()(int rank, double x) {
    std::unique_lock<std::mutex> lk(m);
    if (failed) throw std::string("another rank failed");
    v[rank] = x;
    const long g = gen;
    if (++arrived == n) {
      result = *std::min_element(v.begin(), v.end());
      arrived = 0;
      gen++;
      cv.notify_all();
      return result;
    }
    cv.wait(lk, [&] { return gen != g || failed; });
    if (failed) throw std::string("another rank failed");
    return result;
  }
  void barrier(int rank) { (void)(*this)(rank, 0.0); }
  void fail() {
    std::lock_guard<std::mutex> lk(m);
    failed = true;
    cv.notify_all();
  }
};

// members [lo, hi) of rank r (blocks differ by at most one member; pam_amd/parallel.py: shard_range)
static void shard_range(int nens, int r, int n, int &lo, int &hi) {
  const int base = nens / n, rem = nens % n;
  lo = r * base + std::min(r, rem);
  hi = lo + base + (r < rem ? 1 : 0);
}

// the stand-alone run has no GCM: after vt_init the variance tendency is a relative growth rate per second of the starting variance
static void vt_set_growth_rate(pam::PamCoupler &coupler, double rate) {
  auto &dm = coupler.get_data_manager_device_readwrite();
  const size_t n = (size_t)coupler.get_nz() * coupler.get_nens();
  std::vector<real> h(n);
  const char *q[3] = {"t", "q", "u"};
  for (int i = 0; i < (coupler.get_option<bool>("crm_vt_u") ? 3 : 2); i++) {
    if (hipMemcpy(h.data(), dm.get<real const, 2>(std::string("vt_var_start_") + q[i]).data(), n * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
    for (auto &v : h) v = rate * v;
    if (hipMemcpy(dm.get<real, 2>(std::string("vt_tend_") + q[i]).data(), h.data(), n * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
  }
}

struct Job {
  int nens, nx, ny, nz, nt, nsteps;
  bool mode_a, with_sponge, with_micro, halo_roundtrip, has_consts;
  double geo[3], consts[6];
  std::vector<real> zint;
  std::vector<unsigned char> flags;
  int64_t idWV;
  int nens_in = 0;                           // members in the input file; member e of the run is input member e % nens_in, tile e / nens_in
  std::vector<std::vector<real>> raw;        // the input: density_dry, uvel, vvel, wvel, temp, tracers...: (nz,ny,nx,nens_in) each
  bool want_output = true;
  std::vector<std::vector<real>> fields;     // the output, same order: (nz,ny,nx,nens) each (only when want_output)
  std::vector<real> precl;                   // (ny,nx,nens), Kessler only
  int bench_steps = 0, bench_warmup = 0;
  bool accelerate = false, accel_uv = false;
  double accel_factor = 0, accel_max_ttend = 5.0;
  int accel_crm_steps = 0, accel_ceased = 0;   // out (rank 0)
  bool vt = false, vt_u = false;
  double vt_rate = 0, vt_limit = 0.05;
  bool hyperdiff = false;
  double hyperdiff_tau = 0;
};

struct BenchResult { double seconds = 0; long substeps = 0; };

// One rank = one device, one coupler, one dycore: the reference driver's call sequence on the members [lo, hi).
static void run_rank(Job &J, int rank, int world, int ndev, HostMin &hmin, BenchResult &bench, std::string &name_out) {
  if (hipSetDevice(rank % ndev) != hipSuccess) endrun("hipSetDevice failed");
  int lo, hi;
  shard_range(J.nens, rank, world, lo, hi);
  const int ne = hi - lo, nx = J.nx, ny = J.ny, nz = J.nz, nt = J.nt;
  if (ne < 1) endrun("ERROR: more ranks than ensemble members");
  const size_t ncol = (size_t)nz * ny * nx, ncell = ncol * ne;
  pam::PamCoupler coupler;
  coupler.set_option<real>("crm_dt", J.geo[2]);
  coupler.allocate_coupler_state(nz, ny, nx, ne);                          // driver.cpp:177
  coupler.set_grid(J.geo[0], J.geo[1], J.zint);                            // driver.cpp:180
  // what micro.init()/sgs.init() do for the dycore: constants + tracer registration, BEFORE dycore.init (driver.cpp:189-191)
  const char *cn[6] = {"R_d", "cp_d", "R_v", "cp_v", "p0", "grav"};
  if (J.has_consts) for (int i = 0; i < 6; i++) coupler.set_option<real>(cn[i], J.consts[i]);
  Microphysics micro;
  if (J.with_micro) {
    micro.init(coupler);                                                   // driver.cpp:189
  } else {
    for (int t = 0; t < nt; t++)
      coupler.add_tracer(t == J.idWV ? "water_vapor" : "tracer_" + std::to_string(t), "", J.flags[2 * t] != 0, J.flags[2 * t + 1] != 0);
  }
  Dycore dycore;
  dycore.init(coupler);                                                    // driver.cpp:191
  if (rank == 0) name_out = dycore.dycore_name();                          // driver.cpp:203
  auto &dm = coupler.get_data_manager_device_readwrite();
  std::vector<real> buf(ncell);
  std::vector<std::string> names = {"density_dry", "uvel", "vvel", "wvel", "temp"};
  for (auto &n : coupler.get_tracer_names()) names.push_back(n);
  for (size_t f = 0; f < names.size(); f++) {                              // this rank's members of every field
    const real *src = J.raw[f].data();
    for (size_t c = 0; c < ncol; c++)
      for (int e = 0; e < ne; e++) {
        const int eg = lo + e, tile_i = eg / J.nens_in;                    // tile t gets +t mK on temp: no two CRMs are equal
        buf[c * ne + e] = src[c * J.nens_in + (eg - tile_i * J.nens_in)] + ((f == 4) ? 1.0e-3 * tile_i : 0.0);
      }
    if (hipMemcpy(dm.get<real, 4>(names[f]).data(), buf.data(), ncell * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
  }
#ifdef PAMC_DYCORE
  dycore.pre_time_loop(coupler);                                           // driver.cpp:225-227
#else
  if (!J.mode_a) coupler.set_option<bool>("balance_hydrostasis_with_gravity", false);   // after init(), SURVEY 8c
  dycore.declare_current_profile_as_hydrostatic(coupler);                  // the host model does this once per GCM step
  if (J.halo_roundtrip) {
    // the two converts with the reference's own argument lists (awfl/Dycore.h:1336-1338, :1281-1283), as E3SM's pam_driver
    // calls them: coupler -> the caller's halo'd arrays, coupler fields wiped, arrays -> coupler
    const int hs = 3;
    const std::vector<int> hdims = {nz + 2 * hs, ny + 2 * hs, nx + 2 * hs, ne};
    size_t nh = 1;
    for (int d : hdims) nh *= d;
    real *ps = nullptr, *pt = nullptr;
    if (hipMalloc((void **)&ps, 5 * nh * sizeof(real)) != hipSuccess || hipMalloc((void **)&pt, (size_t)nt * nh * sizeof(real)) != hipSuccess) endrun("hipMalloc");
    real5d state(ps, {5, hdims[0], hdims[1], hdims[2], hdims[3]}), tracers(pt, {nt, hdims[0], hdims[1], hdims[2], hdims[3]});
    dycore.convert_coupler_to_dynamics(coupler, state, tracers);
    for (auto &n : names) (void)hipMemsetAsync(dm.get<real, 4>(n).data(), 0xFF, ncell * sizeof(real), 0);   // NaN bit patterns
    dycore.convert_dynamics_to_coupler(coupler, realConst5d(ps, state.dims()), realConst5d(pt, tracers.dims()));
    if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
    (void)hipFree(ps); (void)hipFree(pt);
  }
#endif
  if (J.hyperdiff) modules::hyperdiffusion_init(coupler, J.hyperdiff_tau);
  auto one_step = [&]() {
#ifdef PAMC_DYCORE
    coupler.run_module("dycore", [&](pam::PamCoupler &c) { dycore.timeStep(c); });      // driver.cpp:248
#else
    if (world == 1) {
      coupler.run_module("dycore", [&](pam::PamCoupler &c) { dycore.timeStep(c); });    // driver.cpp:248
    } else {
      // the dynamics step of the WHOLE ensemble (awfl/Dycore.h:141-145 takes the minimum over every member): this device's
      // minimum, then the minimum over the ranks' N host doubles
      coupler.run_module("dycore", [&](pam::PamCoupler &c) {
        const real dt_all = hmin(rank, dycore.compute_time_step(c));
        dycore.timeStep(c, dt_all);
      });
    }
    bench.substeps += dycore.last_ncycles();
#endif
    if (J.with_sponge) coupler.run_module("sponge_layer", modules::sponge_layer);       // driver.cpp:250
    if (J.hyperdiff) coupler.run_module("hyperdiffusion", [](pam::PamCoupler &c) { modules::hyperdiffusion(c); });
    if (J.with_micro) {                                                                  // driver.cpp:253
      if (world == 1) {
        coupler.run_module("micro", [&](pam::PamCoupler &c) { micro.timeStep(c); });
      } else {
        // Kessler's sedimentation sub-cycle count is a reduction over ALL members as well (rainsplit = ceil(dt / minval(dt2d)),
        // physics/micro/kessler/Microphysics.h:385-390): this shard's stable step, the minimum over the ranks, one count for all
        coupler.run_module("micro", [&](pam::PamCoupler &c) {
          const real dt_max_all = hmin(rank, micro.max_stable_dt(c));
          const real crm_dt = c.get_option<real>("crm_dt");
          const int rainsplit = std::max(1, (int)std::ceil(crm_dt / dt_max_all));
          micro.timeStep(c, rainsplit);
        });
      }
    }
  };
  // --vt: the file's steps are ONE GCM step; the forcing closes every CRM step with the model time the step counts
  const bool vt = J.vt && J.bench_steps == 0;
  if (vt) {
    coupler.set_option<real>("gcm_physics_dt", J.nsteps * J.geo[2]);
    coupler.set_option<bool>("crm_vt_u", J.vt_u);
    coupler.set_option<real>("crm_vt_scale_limit", J.vt_limit);
    coupler.run_module("vt_init", modules::vt_init);
    vt_set_growth_rate(coupler, J.vt_rate);
  }
  auto vt_step = [&](int weight) {
    if (vt) coupler.run_module("vt_apply_forcing", [&](pam::PamCoupler &c) { modules::vt_apply_forcing(c, weight * J.geo[2]); });
  };
  if (J.bench_steps > 0) {
    for (int s = 0; s < J.bench_warmup; s++) one_step();
    if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
    hmin.barrier(rank);
    bench.substeps = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < J.bench_steps; s++) one_step();
    if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
    hmin.barrier(rank);
    bench.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  } else if (J.accelerate) {
    coupler.set_option<real>("crm_accel_factor", J.accel_factor);
    coupler.set_option<bool>("crm_accel_uv", J.accel_uv);
    coupler.set_option<real>("crm_accel_max_ttend", J.accel_max_ttend);
    modules::MsaClock clock(J.nsteps, J.accel_factor);
    coupler.run_module("msa_init", modules::msa_init);
    int steps = 0;
    while (!clock.done()) {
      const bool accel = clock.accelerating();                                           // the same on every rank: the flag is global
      if (accel) coupler.run_module("msa_diagnose", modules::msa_diagnose);
      one_step();
      bool cease = false;
      if (accel)
        coupler.run_module("msa_accelerate", [&](pam::PamCoupler &c) {
          cease = modules::msa_accelerate(c, [&](int mine) { return world == 1 ? mine : (int)-hmin(rank, -(double)mine); });
        });
      vt_step(clock.advance(cease));
      steps++;
    }
    if (rank == 0) { J.accel_crm_steps = steps; J.accel_ceased = clock.ceased() ? 1 : 0; }
  } else {
    for (int s = 0; s < J.nsteps; s++) { one_step(); vt_step(1); }
  }
  if (vt) coupler.run_module("vt_compute_feedback", modules::vt_compute_feedback);
  if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
  for (size_t f = 0; f < names.size() && J.want_output; f++) {
    if (hipMemcpy(buf.data(), dm.get<real, 4>(names[f]).data(), ncell * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
    real *dst = J.fields[f].data();
    for (size_t c = 0; c < ncol; c++) std::memcpy(&dst[c * J.nens + lo], &buf[c * ne], ne * sizeof(real));
  }
  if (J.with_micro && J.want_output) {
    const size_t n2 = (size_t)ny * nx;
    if (hipMemcpy(buf.data(), dm.get<real, 3>("precl").data(), n2 * ne * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
    for (size_t c = 0; c < n2; c++) std::memcpy(&J.precl[c * J.nens + lo], &buf[c * ne], ne * sizeof(real));
  }
  dycore.finalize(coupler);                                                // driver.cpp:285
}

// ------------------------------------------------------------------------------------------------------------------------------
//   driver --yaml <input.yaml> [--nens N] [--steps S] [--check] [--sat-adjust] [--surface-friction TAU BFLX] [--validate] [--diag PATH] [--stats PATH] [--edges PATH]
//          [--radiation RAD_NX RAD_NY PATH] [--accelerate A [--accel-uv] [--accel-max-ttend X]] [--vt RATE PATH [--vt-u] [--vt-limit L]]
//          [--hyperdiff TAU] [--sgs-smag CS PRANDTL] [--sgs-tke CS CK] [--sgs-horizontal] [--sgs-moist] [--sfc-fluxes SHF LHF] [--surface SST [DEPTH]] [--ls-forcing PATH [--coriolis F]] [--esmt [KMAX]] [--radiation-gray [EVERY]] [--shortwave COSZEN [ALBEDO]] [--micro-ice] [--gcm-handoff RAD_NX RAD_NY PATH] [--column-diag PATH]
//          [--flux-profiles PATH] <output.bin | ->
// The reference driver's OWN flow from its own kind of input file (standalone/mmf_simplified/driver.cpp:79-297; the flat
// `key : value` YAML files under standalone/mmf_simplified/inputs/): sim_time, crm_nx, crm_ny, nens, xlen, ylen, dt_gcm, dt_crm_phys,
// out_freq, vcoords [, crm_nz, zlen, idealized, apply_sponge, initData].  What runs, in the reference's order:
//   allocate_coupler_state -> set_grid -> micro.init -> sgs.init -> dycore.init [-> initData on the device when `idealized`] ->
//   initialize_from_supercell_column (driver.cpp:19-77: supercell_init column -> gcm_* columns -> broadcast_initial_gcm_column ->
//   perturb_temperature, all on the device) when not idealized -> per GCM step { declare_current_profile_as_hydrostatic (what E3SM's
//   MMF driver does once per GCM step; the standalone reference never calls it and runs on uninitialised variable_gravity);
//   per CRM step { [radiation ->] dycore -> sponge_layer -> micro } }.
// Not run: P3 and SHOC (the CI build's micro / sgs; SCREAM's numerics are out of scope; their coupling layers are built: physics/micro/p3_amd/Microphysics.h, physics/sgs/shoc_amd/SGS.h) -- Kessler stands in as the microphysics here -- and
// modules::*_gcm_forcing_tendencies, whose field list is P3's tracer set (pam_core/modules/gcm_forcing.h:33-42).
// vcoords: "uniform" (driver.cpp:135-153, with crm_nz and zlen) or the reference's file name `vcoords_equal_<N>_<H>km.nc` -- netCDF-4,
// unreadable here; its contents are what the name says (read from the raw bytes of the reference's copy: 51 interfaces 0, 400, ...,
// 20000 m for vcoords_equal_50_20km.nc): N equal levels up to H km.
// --nens overrides the file's ensemble size, --steps stops after S CRM steps, --check switches the dycore's conservation check on
// (Dycore.h:224-251) and the last stdout line is a JSON object with the run's statistics.  --dump-init PATH (a debug flag, like --sync)
// writes the state the first CRM step starts from, after every init, to PATH: the fields of the output file in its order, without precl.
static std::map<std::string, std::string> read_flat_yaml(const std::string &file) {
  std::ifstream in(file);
  if (!in) die("cannot open the YAML input");
  std::map<std::string, std::string> kv;
  std::string line;
  auto trim = [](std::string v) {
    auto a = v.find_first_not_of(" \t\r\""), b = v.find_last_not_of(" \t\r\"");
    return a == std::string::npos ? std::string() : v.substr(a, b - a + 1);
  };
  while (std::getline(in, line)) {
    auto hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    auto colon = line.find(':');
    if (colon == std::string::npos) continue;
    kv[trim(line.substr(0, colon))] = trim(line.substr(colon + 1));
  }
  return kv;
}

// driver.cpp:19-77
static void initialize_from_supercell_column(std::vector<real> const &zint_in, pam::PamCoupler &coupler) {
  const int nz = coupler.get_nz(), nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  const real R_d = coupler.get_option<real>("R_d"), R_v = coupler.get_option<real>("R_v"), grav = coupler.get_option<real>("grav");
  double *zdev = nullptr, *cols = nullptr;
  if (hipMalloc((void **)&zdev, (nz + 1) * sizeof(double)) != hipSuccess || hipMalloc((void **)&cols, (size_t)6 * nz * sizeof(double)) != hipSuccess) endrun("hipMalloc");
  if (hipMemcpy(zdev, zint_in.data(), (nz + 1) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
  // rho_d, uvel, vvel, wvel, temp, rho_v columns (supercell_init.h:7-135)
  if (pam_amd_supercell_init(nz, zdev, R_d, R_v, grav, cols, cols + nz, cols + 2 * nz, cols + 3 * nz, cols + 4 * nz, cols + 5 * nz, nullptr))
    endrun(pam_amd_awfl_last_error());
  std::vector<double> h((size_t)6 * nz), col((size_t)nz * nens);
  if (hipMemcpy(h.data(), cols, h.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
  auto put = [&](char const *name, int f) {                                  // driver.cpp:55-69: every member gets the column
    for (int k = 0; k < nz; k++)
      for (int e = 0; e < nens; e++) col[(size_t)k * nens + e] = f < 0 ? 0.0 : h[(size_t)f * nz + k];
    if (hipMemcpy(dm.get<real, 2>(name).data(), col.data(), col.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
  };
  put("gcm_density_dry", 0); put("gcm_uvel", 1); put("gcm_vvel", 2); put("gcm_wvel", 3); put("gcm_temp", 4); put("gcm_water_vapor", 5);
  put("ref_density_dry", 0); put("ref_density_vapor", 5); put("ref_density_liq", -1); put("ref_density_ice", -1); put("ref_temp", 4);
  (void)hipFree(zdev); (void)hipFree(cols);
  modules::broadcast_initial_gcm_column(coupler);                            // driver.cpp:72
  int *seeds = nullptr;                                                      // driver.cpp:74-76: int1d seeds("seeds", nens); seeds = 0
  if (hipMalloc((void **)&seeds, nens * sizeof(int)) != hipSuccess || hipMemset(seeds, 0, nens * sizeof(int)) != hipSuccess) endrun("hipMalloc");
  modules::perturb_temperature(coupler, intConst1d(seeds, {nens}));
  if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
  (void)hipFree(seeds);
}

#ifndef PAMC_DYCORE
struct YamlDebug {                                                                  // bisection switches (tools/repro_ci_run.py has the Python twin)
  bool no_micro = false, no_sponge = false, sync = false;
  std::string dump_init;      // --dump-init PATH: the state the first CRM step starts from, the fields in the output file's order
};
// opt-in modules of the CRM step (off: the run is the one above, byte for byte):
//   --sat-adjust               modules::saturation_adjustment after micro
//   --surface-friction TAU BFLX  modules::surface_friction_init once (every member: tau = TAU, bflx = BFLX), then
//                              modules::compute_surface_friction every CRM step after the sponge layer
//   --stats PATH               the CRM -> GCM statistics of E3SM's MMF loop: modules::time_average_init at the start of every GCM
//                              step on the state, the tracers and precl; modules::time_average_accumulate after the last module of
//                              every CRM step; modules::horizontal_average of the "<var>_time_average" entries at the end of every
//                              GCM step (and of a run cut short by --steps).  The (nz,nens) profiles go to PATH as JSON, every value
//                              printed with %.17g (exact round trip); nothing else of the run changes.
//   --edges PATH               at the end of the run: "temp" on the nz+1 vertical interfaces (pam::VerticalInterp<5>, zero gradient at
//                              both ends), (nz+1,ny,nx,nens) raw fp64 to PATH; nothing else of the run changes.
//   --radiation RAD_NX RAD_NY PATH  the forced Radiation plug-in: PATH holds "rad_enthalpy_tend", raw fp64 (nz,rad_ny,rad_nx,nens), read
//                              once after the init; Radiation::timeStep runs FIRST in every CRM step, before the dycore, so that the
//                              dynamics see the heated state (no driver of the reference calls Radiation: the position is this
//                              project's decision).
//   --validate                 dm.validate_all() (DataManager.h:411) after the last module of every CRM step: NaNs and infinities in
//                              the double and float entries, negative values in the double, float, int and long long entries
//                              registered positive-definite (every other type is not looked at), reported on stderr; one device scan and one synchronisation per step; stdout and the
//                              output file are those of a run without it.
//   --diag PATH                one JSON line per OUTPUT step (where the "Etime , dtphys, maxw" line is printed) to PATH: for density_dry,
//                              uvel, vvel, wvel, temp and every tracer the least and the greatest element with their flat indices, the
//                              number of NaNs and the reproducible sum, of the whole field ("whole") and of every ensemble member
//                              ("members"), taken on the device by two scans (pam_amd_field_diagnostics) without copying a field;
//                              stdout and the output file are those of a run without it.
//   --accelerate A [--accel-uv] [--accel-max-ttend X]   CRM mean-state acceleration (modules/mean_state_acceleration.h) with
//                              crm_accel_factor = A: modules::msa_init at the start of every GCM step, modules::msa_diagnose FIRST in
//                              every CRM step, modules::msa_accelerate after its last module; the CRM loop runs on modules::MsaClock, so
//                              a GCM step takes nsteps_crm_phys / (1 + A) CRM steps (1 + A must divide it) unless the acceleration ceases,
//                              and --stats weighs every step by the clock's count.  Without it the loop is the one above.
//   --hyperdiff TAU            horizontal hyperdiffusion (modules/hyperdiffusion.h): modules::hyperdiffusion_init(coupler, TAU) once, then
//                              modules::hyperdiffusion every CRM step after the sponge layer and the surface friction and before the
//                              physics; composes with --accelerate and --vt
//   --sgs-smag CS PRANDTL      the native Smagorinsky SGS closure (physics/sgs/smag_amd/SGS.h) in the SGS slot of the CRM loop: its init in
//                              place of the none class's, its timeStep every CRM step after the sponge layer, the surface friction and the
//                              hyperdiffusion and before the microphysics.  With --surface-friction the fluxes that module computes are
//                              the lower boundary condition of uvel and vvel; composes with every other flag
//   --sgs-tke CS CK            the native prognostic-TKE closure (physics/sgs/tke_amd/SGS.h) in the same slot, and not with --sgs-smag: its
//                              init registers the tracer "tke" before the dycore's, so the dycore transports it; one "sgs tke:" line per
//                              output step with the mass-weighted mean of tke / rho, the extremes of tke = rho e and the greatest tk, from
//                              the field diagnostics' scan (nothing is copied to the host).  --sgs-moist, --sfc-fluxes and --surface
//                              accept either closure (the options are then sgs_tke_moist and sgs_tke_surface_fluxes).
//   --sgs-horizontal           with --sgs-smag or --sgs-tke: option sgs_smag_horizontal / sgs_tke_horizontal, so the closure also mixes along
//                              x and y (pam_amd_sgs_diffuse_horizontal between the coefficients and the vertical solve, with the same tk
//                              and tkh clipped at kcap = 0.25 / (dt (1/dx^2 + 1/dy^2))); one "sgs horizontal:" line per output step with
//                              kcap and the greatest tk and tkh, from the field diagnostics' scan (nothing is copied to the host).
//                              Composes with every other flag
//   --sgs-moist                with --sgs-smag: option sgs_smag_moist, so the closure's stability carries the condensate loading and is
//                              the saturated one inside cloud (the species of option "micro")
//   --surface SST [DEPTH]      with --sgs-smag, and not with --sfc-fluxes: bulk surface fluxes over a slab ocean (modules/surface_fluxes.h).
//                              modules::surface_fluxes_init(coupler, SST, DEPTH) once, option sgs_smag_surface_fluxes, then
//                              modules::compute_surface_fluxes every CRM step after the sponge layer and before the surface friction and
//                              the SGS: "sfc_shf" and "sfc_lhf" from the lowest level and "sfc_temp", which starts at SST [K] and, with
//                              DEPTH > 0 [m of water], takes the net energy (with --radiation-gray [--shortwave] the radiation too).  One
//                              "surface:" line per output step with the means of the three.  Composes with the rest.
//   --ls-forcing PATH [--coriolis F]  large-scale forcing (modules/large_scale_forcing.h).  PATH is a raw float64 file of (rows, crm_nz),
//                              rows <= 12, every row one profile applied to every member, in this order: wsub [m/s], temp_tend [K/s],
//                              qv_tend [1/s], ug, vg [m/s], nudge_temp [K], nudge_qv [1], nudge_u, nudge_v [m/s], nudge_rate_temp,
//                              nudge_rate_qv, nudge_rate_uv [1/s].  A row that is all NaN, or missing at the end, means "absent".
//                              --coriolis F sets "ls_fcor" of every member [1/s] and needs the rows ug and vg.
//                              modules::ls_forcing_init once, then modules::ls_forcing every CRM step after the sponge layer and before
//                              the surface fluxes.  One "ls forcing:" line per output step with the domain means of uvel and vvel and
//                              the mean temp of level 0.  Composes with the rest (--surface, --sgs-smag, --radiation-gray, --hyperdiff,
//                              --accelerate, --vt).
//   --sfc-fluxes SHF LHF       with --sgs-smag: option sgs_smag_surface_fluxes; "sfc_shf" and "sfc_lhf" are filled uniformly, once, with
//                              SHF and LHF (W/m2, positive upward) and enter row 0 of temp and of the vapour in every SGS step.  Both
//                              compose with every other flag
//   --esmt [KMAX]              explicit scalar momentum transport (modules/scalar_momentum.h) on a 2-D CRM (crm_ny == 1): modules::esmt_init
//                              before dycore.init (two more tracers, "esmt_u" and "esmt_v"), the scalars set from the CRM's own level-mean
//                              wind (modules::esmt_set "crm"), then modules::esmt_pgf every CRM step after the sponge layer and before the
//                              SGS, with the wavenumbers 1 .. KMAX (default crm_nx / 2); there is no GCM, so there is no forcing.  Per
//                              output step a line "esmt: etime <s> , u_s <m/s> , v_s <m/s> , max_T_dt <m/s>": the means of esmt_x / rho
//                              over the domain and the largest |T| dt of the last step that was probed (the step before an output).
//                              Composes with the rest.
//   --radiation-gray [EVERY]   the native grey two-stream longwave scheme (physics/radiation/gray_amd/radiation.h) in the radiation slot of
//                              the CRM loop, where --radiation puts the forced class: its timeStep every CRM step before the dycore, the
//                              fluxes recomputed on every EVERY-th step (1 unless given) and the stored heating applied between.  One
//                              "radiation gray:" line per output step with the ensemble-mean OLR and surface downward flux.  Composes
//                              with every other flag but --radiation: there is one slot
//   --shortwave COSZEN [ALBEDO]   with --radiation-gray: option rad_gray_shortwave, the scheme's grey two-stream shortwave under a sun
//                              whose zenith angle has the cosine COSZEN for every member (rad_gray_sw_coszen) over a surface of albedo
//                              ALBEDO (rad_gray_sw_albedo; 0.07 unless given).  The "radiation gray:" line then also carries the mean
//                              rad_sw_down_sfc and rad_sw_up_top.  Refused without --radiation-gray
//   --micro-ice                the native one-moment microphysics with ice (physics/micro/ice_amd/Microphysics.h, option micro = "ice1m") in the
//                              microphysics slot of the CRM loop, where Kessler runs without the flag: its init registers five water
//                              tracers, "precl" and "preci", and its timeStep runs where Kessler's does.  Every module that reads the
//                              condensate takes cloud_liquid and cloud_ice.  One "micro ice:" line per output step with the mean ice water
//                              path [kg/m2], the mean precl and preci [m/s] and the water budget [kg/m2 summed over the columns]: the
//                              total water now, the total at the start and the accumulated surface precipitation.  Composes with every
//                              flag that composes with Kessler
//   --vt RATE PATH [--vt-u] [--vt-limit L]   CRM variance transport (modules/variance_transport.h): modules::vt_init at the start of every GCM
//                              step; there is no GCM here, so vt_tend_x = RATE vt_var_start_x (a relative growth rate per second) for
//                              that GCM step; modules::vt_apply_forcing LAST in every CRM step, after the clock has advanced, with dt =
//                              the step's weight times crm_dt, so that it composes with --accelerate; modules::vt_compute_feedback at the
//                              end of the GCM step.  PATH receives one JSON line per GCM step with var_start, var and feedback of every
//                              quantity as flat (nz,nens) lists, printed with %.17g.  RATE = 0 changes nothing of the run.
//   --gcm-handoff RAD_NX RAD_NY PATH   what the GCM takes back from the CRM (modules/radiation_aggregate.h, modules/crm_feedback.h):
//                              modules::rad_aggregate_init at the start of every GCM step, modules::rad_aggregate after the last module
//                              of every CRM step with the clock's weight (so it composes with --accelerate, --vt and --hyperdiff),
//                              modules::compute_crm_feedback at the end of every GCM step (and of a run cut short by --steps).  The
//                              aggregates (nz,rad_ny,rad_nx,nens) and the feedback's means and tendencies (nz,nens) go to PATH as JSON in
//                              the format of --stats, every value printed with %.17g; nothing else of the run changes.  With --radiation
//                              the two rad grids must be the same.
//   --column-diag PATH         the CRM column diagnostics (modules/column_diagnostics.h): modules::column_diagnostics_init at the start of
//                              every GCM step, modules::column_diagnostics after the last module of every CRM step with the clock's
//                              weight (so it composes with --accelerate, --vt, --hyperdiff, --gcm-handoff and --radiation).  PATH
//                              receives one JSON record (a line) per GCM step with the (nens) lists of diag_cldtot, diag_cldlow,
//                              diag_cldmed, diag_cldhgh, diag_lwp, diag_pw and diag_precip_liq (Kessler has no ice), printed with %.17g;
//                              nothing else of the run changes.
//   --flux-profiles PATH       the CRM flux profiles (modules/flux_profiles.h): modules::flux_profiles_init at the start of every GCM
//                              step, modules::flux_profiles after the last module of every CRM step with the clock's weight (so it
//                              composes with --accelerate, --vt, --hyperdiff, --gcm-handoff, --column-diag and --radiation).  PATH receives
//                              one JSON record (a line) per GCM step: gcm_step, crm_steps, nens, nz and "profiles", name -> nz rows of nens
//                              values of prof_mcup, prof_mcdn, prof_mcuup, prof_mcudn, prof_cld, prof_flux_t, prof_flux_qt, prof_flux_u,
//                              prof_flux_v and prof_tke, printed with %.17g; nothing else of the run changes.
struct YamlModules {
  bool sat_adjust = false, surface_friction = false, radiation = false, validate = false, accelerate = false, accel_uv = false;
  bool micro_ice = false, vt = false, vt_u = false, hyperdiff = false, handoff = false, sgs_smag = false, sgs_tke = false, sgs_horizontal = false, sgs_moist = false, sfc_fluxes = false, radiation_gray = false, shortwave = false, surface = false, ls_forcing = false, coriolis = false, esmt = false;
  int radiation_gray_every = 1, esmt_kmax = -1;
  double sw_coszen = 1, sw_albedo = 0.07;
  double hyperdiff_tau = 0, sgs_cs = 0, sgs_prandtl = 0, sgs_ck = 0, sfc_shf = 0, sfc_lhf = 0, surface_sst = 300, surface_depth = 0, ls_fcor = 0;
  int handoff_rad_nx = 0, handoff_rad_ny = 0;
  std::string handoff_path;
  double tau = 0, bflx = 0, accel_factor = 0, accel_max_ttend = 5.0, vt_rate = 0, vt_limit = 0.05;
  int rad_nx = 0, rad_ny = 0;
  std::string stats, edges, rad_path, diag, vt_path, column_diag, flux_profiles, ls_path;
};

// one JSON number that Python's json module reads back exactly (NaN / Infinity for the non-finite)
static void stats_json_number(std::string &o, double v) {
  char t[40];
  if (std::isnan(v)) std::snprintf(t, sizeof(t), "NaN");
  else if (std::isinf(v)) std::snprintf(t, sizeof(t), v > 0 ? "Infinity" : "-Infinity");
  else std::snprintf(t, sizeof(t), "%.17g", v);
  o += t;
}
// --gcm-handoff: a device array as nested JSON lists, the last dimension innermost
static void handoff_json_array(std::string &o, const real *dev, std::vector<int> const &dims) {
  size_t n = 1;
  for (int d : dims) n *= d;
  std::vector<real> h(n);
  if (hipMemcpy(h.data(), dev, n * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
  std::vector<size_t> inner(dims.size(), 1);      // elements below one index of dimension d
  for (int d = (int)dims.size() - 2; d >= 0; d--) inner[d] = inner[d + 1] * dims[d + 1];
  for (size_t j = 0; j < n; j++) {
    for (size_t d = 0; d < dims.size(); d++)
      if (j % (inner[d] * dims[d]) == 0) o += "[";
    stats_json_number(o, h[j]);
    for (int d = (int)dims.size() - 1; d >= 0; d--)
      if ((j + 1) % (inner[d] * dims[d]) == 0) o += "]";
    if (j + 1 < n) o += ", ";
  }
}
// --diag: one result set of pam::diagnostics::scan as JSON, scalars for the whole field (members = 0), lists per member
static void diag_json(std::string &o, pam::diagnostics::FieldDiagnostics const &d) {
  auto doubles = [&](char const *key, std::vector<double> const &v) {
    o += std::string("\"") + key + "\": " + (d.members ? "[" : "");
    for (size_t m = 0; m < v.size(); m++) { if (m) o += ", "; stats_json_number(o, v[m]); }
    o += d.members ? "], " : ", ";
  };
  auto integers = [&](char const *key, std::vector<long long> const &v, bool last) {
    o += std::string("\"") + key + "\": " + (d.members ? "[" : "");
    for (size_t m = 0; m < v.size(); m++) o += (m ? ", " : "") + std::to_string(v[m]);
    o += std::string(d.members ? "]" : "") + (last ? "" : ", ");
  };
  o += "{";
  doubles("vmin", d.vmin);
  doubles("vmax", d.vmax);
  doubles("vsum", d.vsum);
  integers("argmin", d.argmin, false);
  integers("argmax", d.argmax, false);
  integers("nan_count", d.nan_count, true);
  o += "}";
}
static int run_yaml(const std::string &file, int nens_override, int steps_limit, bool check, const std::string &outfile, YamlDebug dbg = YamlDebug(),
                    YamlModules mods = YamlModules()) {
  auto kv = read_flat_yaml(file);
  auto has = [&](char const *k) { return kv.count(k) > 0; };
  auto num = [&](char const *k, double dflt, bool required = false) {
    if (!has(k)) { if (required) die((std::string("YAML key missing: ") + k).c_str()); return dflt; }
    return std::atof(kv[k].c_str());
  };
  auto flag = [&](char const *k, bool dflt) { return has(k) ? (kv[k] == "true" || kv[k] == "True" || kv[k] == "1") : dflt; };
  const bool idealized = flag("idealized", false);                           // driver.cpp:91-94
  const bool apply_sponge = flag("apply_sponge", !idealized);
  const bool apply_gcm_forcing = flag("apply_gcm_forcing", !idealized);
  const double sim_time = num("sim_time", 0, true);
  const int crm_nx = (int)num("crm_nx", 0, true), crm_ny = (int)num("crm_ny", 0, true);
  const int nens = nens_override > 0 ? nens_override : (int)num("nens", 0, true);
  const double xlen = num("xlen", -1), ylen = num("ylen", -1), zlen = num("zlen", -1);
  double dt_gcm = num("dt_gcm", sim_time), dt_crm_phys = num("dt_crm_phys", 0, true);
  const double out_freq = num("out_freq", -1);
  if (!has("vcoords")) die("YAML key missing: vcoords");
  const std::string vcoords = kv["vcoords"];
  const int nsteps_gcm = (int)std::ceil(sim_time / dt_gcm);                  // driver.cpp:115-118
  dt_gcm = sim_time / nsteps_gcm;
  const int nsteps_crm_phys = (int)std::ceil(dt_gcm / dt_crm_phys);
  dt_crm_phys = dt_gcm / nsteps_crm_phys;
  std::vector<real> zint;
  if (vcoords == "uniform") {                                                // driver.cpp:135-153
    const int crm_nz = (int)num("crm_nz", 0, true);
    if (!(zlen > 0)) die("vcoords: uniform needs zlen");
    const real dz = zlen / (crm_nz - 1);
    zint.resize(crm_nz + 1);
    for (int k = 0; k <= crm_nz; k++) zint[k] = (k == 0) ? 0 : (k == crm_nz ? zlen : k * dz - dz / 2);
  } else {
    int n = 0; double hkm = 0;
    if (std::sscanf(vcoords.c_str(), "vcoords_equal_%d_%lfkm.nc", &n, &hkm) != 2 || n < 3 || !(hkm > 0))
      die("vcoords: only `uniform` and `vcoords_equal_<N>_<H>km.nc` are understood (netCDF is not available here)");
    zint.resize(n + 1);
    for (int k = 0; k <= n; k++) zint[k] = hkm * 1000.0 * k / n;
  }
  const int crm_nz = (int)zint.size() - 1;
  if (!(xlen > 0) || !(ylen > 0)) die("xlen / ylen must be given");
  if (hipSetDevice(0) != hipSuccess) die("no HIP device");
  int rcode = 0;
  try {
    pam::PamCoupler coupler;
    coupler.set_option<real>("gcm_physics_dt", dt_gcm);                      // driver.cpp:122-123
    coupler.set_option<real>("crm_dt", dt_crm_phys);
    if (idealized) coupler.set_option<std::string>("standalone_input_file", file);   // driver.cpp:125-128
    coupler.allocate_coupler_state(crm_nz, crm_ny, crm_nx, nens);            // driver.cpp:177
    coupler.set_grid(xlen, ylen, zint);                                      // driver.cpp:180
    Dycore dycore;
    Microphysics micro;
    MicrophysicsIce micro_ice;
    SGS sgs;
    SGSSmagorinsky sgs_smag;
    SGSTke sgs_tke;
    Radiation rad;
    RadiationGray rad_gray;
    if (mods.micro_ice) micro_ice.init(coupler);                             // --micro-ice: the native scheme with ice in the microphysics slot
    else micro.init(coupler);                                                // driver.cpp:189
    if (mods.sgs_smag || mods.sgs_tke) {                                     // --sgs-smag / --sgs-tke: a native closure in the SGS slot
      if (mods.sgs_smag) {
        coupler.set_option<real>("sgs_smag_cs", mods.sgs_cs);
        coupler.set_option<real>("sgs_smag_prandtl", mods.sgs_prandtl);
        coupler.set_option<bool>("sgs_smag_moist", mods.sgs_moist);
        coupler.set_option<bool>("sgs_smag_surface_fluxes", mods.sfc_fluxes || mods.surface);
        if (mods.sgs_horizontal) coupler.set_option<bool>("sgs_smag_horizontal", true);
        sgs_smag.init(coupler);
      } else {                                                               // registers the tracer "tke" before the dycore takes its table
        coupler.set_option<real>("sgs_tke_cs", mods.sgs_cs);
        coupler.set_option<real>("sgs_tke_ck", mods.sgs_ck);
        coupler.set_option<bool>("sgs_tke_moist", mods.sgs_moist);
        coupler.set_option<bool>("sgs_tke_surface_fluxes", mods.sfc_fluxes || mods.surface);
        if (mods.sgs_horizontal) coupler.set_option<bool>("sgs_tke_horizontal", true);
        sgs_tke.init(coupler);
      }
      if (mods.sfc_fluxes) {                                                 // --sfc-fluxes: the two entries, uniformly, once
        auto &sdm = coupler.get_data_manager_device_readwrite();
        std::vector<real> h((size_t)crm_ny * crm_nx * nens);
        for (int q = 0; q < 2; q++) {
          std::fill(h.begin(), h.end(), (real)(q == 0 ? mods.sfc_shf : mods.sfc_lhf));
          if (hipMemcpy(sdm.get<real, 3>(q == 0 ? "sfc_shf" : "sfc_lhf").data(), h.data(), h.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess)
            endrun("memcpy");
        }
      }
    } else sgs.init(coupler);                                                // driver.cpp:190 (the reference's CI build: SHOC with P3; their numerics are out of scope, their coupling layers are physics/sgs/shoc_amd and physics/micro/p3_amd)
    if (mods.esmt) modules::esmt_init(coupler, mods.esmt_kmax);              // --esmt: two more tracers, before the dycore takes its table
    dycore.init(coupler);                                                    // driver.cpp:191
    if (mods.radiation_gray) {                                               // --radiation-gray: the native scheme in the radiation slot
      coupler.set_option<int>("rad_gray_every", mods.radiation_gray_every);
      if (mods.shortwave) {                                                  // --shortwave: the sun on, the same for every member
        coupler.set_option<bool>("rad_gray_shortwave", true);
        coupler.set_option<real>("rad_gray_sw_coszen", mods.sw_coszen);
        coupler.set_option<real>("rad_gray_sw_albedo", mods.sw_albedo);
      }
      rad_gray.init(coupler);
    }
    if (mods.radiation) {
      coupler.set_option<int>("rad_nx", mods.rad_nx);
      coupler.set_option<int>("rad_ny", mods.rad_ny);
      rad.init(coupler);
      auto tend = coupler.get_data_manager_device_readwrite().get<real, 4>("rad_enthalpy_tend");
      std::vector<real> h(tend.size());
      std::ifstream rin(mods.rad_path, std::ios::binary);
      if (!rin) endrun("cannot open the --radiation file");
      rin.read((char *)h.data(), h.size() * sizeof(real));
      if (!rin || rin.peek() != std::ifstream::traits_type::eof()) endrun("the --radiation file is not (nz,rad_ny,rad_nx,nens) fp64");
      if (hipMemcpy(tend.data(), h.data(), h.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("memcpy");
    }
    std::printf("Dycore: %s\nMicro : %s\nSGS   : %s\n\n", dycore.dycore_name(), (mods.micro_ice ? micro_ice.micro_name() : micro.micro_name()).c_str(),
                mods.sgs_smag ? sgs_smag.sgs_name().c_str() : mods.sgs_tke ? sgs_tke.sgs_name().c_str() : "none (SHOC is out of scope)");   // driver.cpp:203-205
    std::printf("crm_nx:   %d\ncrm_ny:   %d\ncrm_nz:   %d\nxlen (m): %g\nylen (m): %g\n", crm_nx, crm_ny, crm_nz, xlen, ylen);
    if (apply_gcm_forcing) std::printf("apply_gcm_forcing: not run (modules::gcm_forcing works on P3's tracer set; P3 is out of scope)\n");
    if (!idealized) initialize_from_supercell_column(zint, coupler);        // driver.cpp:220-222
    if (check) dycore.set_debug_conservation(true);
    if (mods.accelerate) {
      coupler.set_option<real>("crm_accel_factor", mods.accel_factor);
      coupler.set_option<bool>("crm_accel_uv", mods.accel_uv);
      coupler.set_option<real>("crm_accel_max_ttend", mods.accel_max_ttend);
    }
    if (mods.hyperdiff) modules::hyperdiffusion_init(coupler, mods.hyperdiff_tau);
    std::string handoff_steps;
    if (mods.handoff) {
      if (mods.radiation && (mods.rad_nx != mods.handoff_rad_nx || mods.rad_ny != mods.handoff_rad_ny))
        endrun("--radiation and --gcm-handoff must name the same rad grid");
      coupler.set_option<int>("rad_nx", mods.handoff_rad_nx);
      coupler.set_option<int>("rad_ny", mods.handoff_rad_ny);
      coupler.run_module("crm_feedback_init", modules::crm_feedback_init);
    }
    std::ofstream coldiag_out;
    if (!mods.column_diag.empty()) {
      coldiag_out.open(mods.column_diag);
      if (!coldiag_out) endrun("cannot open the --column-diag file");
    }
    std::ofstream fluxprof_out;
    if (!mods.flux_profiles.empty()) {
      fluxprof_out.open(mods.flux_profiles);
      if (!fluxprof_out) endrun("cannot open the --flux-profiles file");
    }
    std::ofstream vt_out;
    if (mods.vt) {
      coupler.set_option<bool>("crm_vt_u", mods.vt_u);
      coupler.set_option<real>("crm_vt_scale_limit", mods.vt_limit);
      vt_out.open(mods.vt_path);
      if (!vt_out) endrun("cannot open the --vt file");
    }
    auto &dm = coupler.get_data_manager_device_readwrite();
    double *sf_in = nullptr;                                                 // tau_in, bflx_in of surface_friction_init: (2, nens)
    if (mods.surface_friction) {
      std::vector<real> h((size_t)2 * nens);
      for (int e = 0; e < nens; e++) { h[e] = mods.tau; h[nens + e] = mods.bflx; }
      if (hipMalloc((void **)&sf_in, h.size() * sizeof(real)) != hipSuccess ||
          hipMemcpy(sf_in, h.data(), h.size() * sizeof(real), hipMemcpyHostToDevice) != hipSuccess) endrun("hipMalloc");
      realConst1d tau_in(sf_in, {nens}), bflx_in(sf_in + nens, {nens});
      coupler.run_module("surface_friction_init", [&](pam::PamCoupler &c) { modules::surface_friction_init(c, tau_in, bflx_in); });
    }
    if (mods.surface)                                                        // --surface: after the friction's init, whose z0 it takes
      coupler.run_module("surface_fluxes_init", [&](pam::PamCoupler &c) { modules::surface_fluxes_init(c, mods.surface_sst, mods.surface_depth); });
    if (mods.ls_forcing) {                                                   // --ls-forcing: the rows of the file, an all-NaN row absent
      std::ifstream in(mods.ls_path, std::ios::binary);
      if (!in) endrun("cannot open the --ls-forcing file");
      in.seekg(0, std::ios::end);
      const size_t bytes = (size_t)in.tellg(), row = (size_t)crm_nz * sizeof(double);
      if (bytes == 0 || bytes % row != 0 || bytes / row > 12) endrun("the --ls-forcing file must hold 1 to 12 rows of crm_nz float64 values");
      in.seekg(0);
      modules::LsProfiles P;
      std::vector<real> *slots[12] = {&P.wsub, &P.temp_tend, &P.qv_tend, &P.ug, &P.vg, &P.nudge_temp, &P.nudge_qv, &P.nudge_u, &P.nudge_v,
                                      &P.nudge_rate_temp, &P.nudge_rate_qv, &P.nudge_rate_uv};
      for (size_t r = 0; r < bytes / row; r++) {
        std::vector<real> v(crm_nz);
        in.read((char *)v.data(), row);
        bool some = false;
        for (real x : v) some = some || x == x;
        if (some) *slots[r] = v;
      }
      if (mods.coriolis) P.fcor = {mods.ls_fcor};
      coupler.run_module("ls_forcing_init", [&](pam::PamCoupler &c) { modules::ls_forcing_init(c, P); });
    }
    if (mods.esmt) coupler.run_module("esmt_set", [](pam::PamCoupler &c) { modules::esmt_set(c, "crm"); });   // from the CRM's own level-mean wind
    double esmt_max_t_dt = 0;
    const size_t ncell = (size_t)crm_nz * crm_ny * crm_nx * nens;
    std::vector<real> buf(ncell);
    auto fetch = [&](std::string const &name) {
      if (hipMemcpy(buf.data(), dm.get<real const, 4>(name).data(), ncell * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
    };
    if (!dbg.dump_init.empty()) {                                            // --dump-init: what the loop starts from, before the first step
      std::ofstream di(dbg.dump_init, std::ios::binary);
      if (!di) endrun("cannot open the --dump-init file");
      std::vector<std::string> init_names = {"density_dry", "uvel", "vvel", "wvel", "temp"};
      for (auto &n : coupler.get_tracer_names()) init_names.push_back(n);
      for (auto &n : init_names) {
        fetch(n);
        di.write((char *)buf.data(), ncell * sizeof(real));
      }
      if (!di) endrun("cannot write the --dump-init file");
    }
    // --stats: the fields averaged over each GCM step, and their profiles as JSON
    const bool stats = !mods.stats.empty();
    std::vector<std::string> stat_names = {"density_dry", "uvel", "vvel", "wvel", "temp"};
    for (auto &n : coupler.get_tracer_names()) stat_names.push_back(n);
    stat_names.push_back("precl");
    std::vector<std::tuple<std::string, bool>> stat_havg;
    for (auto &n : stat_names) stat_havg.emplace_back(n + "_time_average", n != "precl");
    std::string stats_steps;
    // --diag: the fields looked at, and the file
    std::vector<std::string> diag_names = {"density_dry", "uvel", "vvel", "wvel", "temp"};
    for (auto &n : coupler.get_tracer_names()) diag_names.push_back(n);
    std::ofstream diag_out;
    if (!mods.diag.empty()) {
      diag_out.open(mods.diag);
      if (!diag_out) endrun("cannot open the --diag file");
    }
    double etime_gcm = 0, maxw_all = 0, cons_max_rel = 0;
    // --micro-ice: the water budget.  Total water [kg/m2 summed over the columns] at the start, and the surface precipitation since
    long double ice_water_start = 0, ice_precip_sum = 0;
    if (mods.micro_ice) ice_water_start = micro_ice.compute_total_mass(coupler);
    auto mean2d = [&](char const *name) {                                    // the mean of a (ny,nx,nens) entry
      const size_t n2 = (size_t)crm_ny * crm_nx * nens;
      std::vector<real> h(n2);
      if (hipMemcpy(h.data(), dm.get<real const, 3>(name).data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
      long double sum = 0;
      for (real v : h) sum += v;
      return (double)(sum / n2);
    };
    int num_out = 0, crm_steps = 0, accel_steps = 0, accel_ceased_gcm_steps = 0;
    long substeps = 0, cons_violations = 0;
    bool stop = false;
    std::string maxw_series;
    for (int step_gcm = 0; step_gcm < nsteps_gcm && !stop; ++step_gcm) {
      if (stats) coupler.run_module("time_average_init", [&](pam::PamCoupler &c) { modules::time_average_init(c, stat_names); });
      dycore.declare_current_profile_as_hydrostatic(coupler);               // (E3SM's MMF driver: once per GCM step)
      int crm_steps_gcm = 0;
      // the CRM loop runs on the clock: without --accelerate every step counts 1 and the loop is step_crm_phys = 0 .. nsteps_crm_phys - 1
      modules::MsaClock clock(nsteps_crm_phys, mods.accelerate ? mods.accel_factor : 0.0);
      if (mods.accelerate) coupler.run_module("msa_init", modules::msa_init);
      if (mods.vt) {
        coupler.run_module("vt_init", modules::vt_init);
        vt_set_growth_rate(coupler, mods.vt_rate);
      }
      if (mods.handoff) coupler.run_module("rad_aggregate_init", modules::rad_aggregate_init);
      if (coldiag_out.is_open()) coupler.run_module("column_diagnostics_init", modules::column_diagnostics_init);
      if (fluxprof_out.is_open()) coupler.run_module("flux_profiles_init", modules::flux_profiles_init);
      while (!clock.done() && !stop) {
        const bool accel = clock.accelerating();
        if (accel) coupler.run_module("msa_diagnose", modules::msa_diagnose);
        if (mods.radiation) coupler.run_module("radiation", [&](pam::PamCoupler &c) { rad.timeStep(c); });
        if (mods.radiation_gray) coupler.run_module("radiation", [&](pam::PamCoupler &c) { rad_gray.timeStep(c); });
        coupler.run_module("dycore", [&](pam::PamCoupler &c) { dycore.timeStep(c); });       // driver.cpp:248
        substeps += dycore.last_ncycles();
        if (check) {
          cons_violations += dycore.conservation_violations();
          cons_max_rel = std::max(cons_max_rel, (double)dycore.conservation_max_rel_diff());
        }
        if (dbg.sync && hipDeviceSynchronize() != hipSuccess) endrun("device error");
        if (apply_sponge && !dbg.no_sponge) coupler.run_module("sponge_layer", modules::sponge_layer);         // driver.cpp:249-251
        if (mods.ls_forcing) coupler.run_module("ls_forcing", [](pam::PamCoupler &c) { modules::ls_forcing(c); });
        if (mods.esmt) {                                                     // --esmt: the pressure force on the two scalars; no GCM, no forcing
          // probed on the step an output follows (any step of an accelerated run): the scalars before and after, for max |T| dt
          const bool probe = out_freq >= 0. && (accel || (step_gcm * dt_gcm + (clock.count() + 1) * dt_crm_phys) / out_freq >= num_out + 1);
          std::vector<real> before[2];
          if (probe)
            for (int x = 0; x < 2; x++) { fetch(x == 0 ? "esmt_u" : "esmt_v"); before[x] = buf; }
          coupler.run_module("esmt_pgf", [](pam::PamCoupler &c) { modules::esmt_pgf(c, -1, false); });
          if (probe) {
            std::vector<real> rho(ncell);
            fetch("density_dry");
            rho = buf;
            fetch("water_vapor");
            for (size_t c = 0; c < ncell; c++) rho[c] += buf[c];
            esmt_max_t_dt = 0;
            for (int x = 0; x < 2; x++) {
              fetch(x == 0 ? "esmt_u" : "esmt_v");
              for (size_t c = 0; c < ncell; c++) {
                const double d = std::fabs((buf[c] - before[x][c]) / rho[c]);
                esmt_max_t_dt = d > esmt_max_t_dt || d != d ? d : esmt_max_t_dt;
              }
            }
          }
        }
        if (mods.surface) coupler.run_module("surface_fluxes", [](pam::PamCoupler &c) { modules::compute_surface_fluxes(c); });
        if (mods.surface_friction) coupler.run_module("surface_friction", modules::compute_surface_friction);
        if (mods.hyperdiff) coupler.run_module("hyperdiffusion", [](pam::PamCoupler &c) { modules::hyperdiffusion(c); });
        if (mods.sgs_smag) coupler.run_module("sgs", [&](pam::PamCoupler &c) { sgs_smag.timeStep(c); });
        if (mods.sgs_tke) coupler.run_module("sgs", [&](pam::PamCoupler &c) { sgs_tke.timeStep(c); });
        if (dbg.sync && hipDeviceSynchronize() != hipSuccess) endrun("device error");
        if (!dbg.no_micro && mods.micro_ice) {
          coupler.run_module("micro", [&](pam::PamCoupler &c) { micro_ice.timeStep(c); });
          const double n2 = (double)crm_ny * crm_nx * nens;                  // 1000 dt (precl + preci) of every column, added up
          ice_precip_sum += (long double)1000.0 * dt_crm_phys * ((long double)mean2d("precl") + (long double)mean2d("preci")) * n2;
        } else
        if (!dbg.no_micro) coupler.run_module("micro", [&](pam::PamCoupler &c) { micro.timeStep(c); });         // driver.cpp:253
        if (mods.sat_adjust) coupler.run_module("saturation_adjustment", modules::saturation_adjustment);
        bool cease = false;
        if (accel) coupler.run_module("msa_accelerate", [&](pam::PamCoupler &c) { cease = modules::msa_accelerate(c); });
        const int weight = clock.advance(cease);
        if (accel && !cease) accel_steps++;
        if (mods.vt) coupler.run_module("vt_apply_forcing", [&](pam::PamCoupler &c) { modules::vt_apply_forcing(c, weight * dt_crm_phys); });
        if (stats) coupler.run_module("time_average_accumulate", [&](pam::PamCoupler &c) { modules::time_average_accumulate(c, stat_names, weight); });
        if (mods.handoff) coupler.run_module("rad_aggregate", [&](pam::PamCoupler &c) { modules::rad_aggregate(c, weight); });
        if (coldiag_out.is_open()) coupler.run_module("column_diagnostics", [&](pam::PamCoupler &c) { modules::column_diagnostics(c, weight); });
        if (fluxprof_out.is_open()) coupler.run_module("flux_profiles", [&](pam::PamCoupler &c) { modules::flux_profiles(c, weight); });
        if (mods.validate) dm.validate_all();
        if (dbg.sync && hipDeviceSynchronize() != hipSuccess) endrun("device error");
        crm_steps++;
        crm_steps_gcm++;
        etime_gcm = step_gcm * dt_gcm + clock.count() * dt_crm_phys;        // driver.cpp:255
        if (out_freq >= 0. && etime_gcm / out_freq >= num_out + 1) {        // driver.cpp:257-271 (the netCDF output itself: out of scope)
          fetch("wvel");
          double maxw = 0;
          for (real v : buf) maxw = std::max(maxw, std::fabs(v));
          if (!(maxw == maxw)) maxw = INFINITY;
          maxw_all = std::max(maxw_all, maxw);
          std::printf("Etime , dtphys, maxw: %g , %g , %10.6g\n", etime_gcm, dt_crm_phys, maxw);
          if (mods.radiation_gray) {                                         // the ensemble-mean (and column-mean) fluxes of the last computation
            const size_t n2 = (size_t)crm_ny * crm_nx * nens;
            std::vector<real> olr(n2), down(n2);
            if (hipMemcpy(olr.data(), dm.get<real const, 3>("rad_olr").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(down.data(), dm.get<real const, 3>("rad_lw_down_sfc").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
              endrun("memcpy");
            double so = 0, sd = 0;
            for (size_t c = 0; c < n2; c++) { so += olr[c]; sd += down[c]; }
            if (!mods.shortwave) std::printf("radiation gray: etime %g , olr %.9g , lw_down_sfc %.9g\n", etime_gcm, so / n2, sd / n2);
            else {
              if (hipMemcpy(olr.data(), dm.get<real const, 3>("rad_sw_down_sfc").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess ||
                  hipMemcpy(down.data(), dm.get<real const, 3>("rad_sw_up_top").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
                endrun("memcpy");
              double ss = 0, st = 0;
              for (size_t c = 0; c < n2; c++) { ss += olr[c]; st += down[c]; }
              std::printf("radiation gray: etime %g , olr %.9g , lw_down_sfc %.9g , sw_down_sfc %.9g , sw_up_top %.9g\n", etime_gcm, so / n2, sd / n2,
                          ss / n2, st / n2);
            }
          }
          if (mods.surface) {                                                // the means over all columns and members, by the reproducible sum of
            std::vector<pam::diagnostics::Item> items;                       // the scan behind DataManager::diagnose, one scan for the three
            for (char const *n : {"sfc_shf", "sfc_lhf", "sfc_temp"})
              items.push_back({n, 0, dm.get<real const, 3>(n).data(), (long long)crm_ny * crm_nx * nens, items.size()});
            auto s3 = pam::diagnostics::scan(items, 0);
            std::printf("surface: etime %g , shf %.9g , lhf %.9g , sfc_temp %.17g\n", etime_gcm, s3[0].mean(), s3[1].mean(), s3[2].mean());
          }
          if (mods.sgs_tke) {                                                // the same scan, nothing copied to the host: e_mean = S tke / S rho (the
            const long long cells = (long long)crm_ny * crm_nx * nens * crm_nz;   // mass-weighted mean of tke / rho), the extremes of tke = rho e, and of tk
            std::vector<pam::diagnostics::Item> items;
            for (char const *n : {"tke", "density_dry", "water_vapor", "tk"}) items.push_back({n, 0, dm.get<real const, 4>(n).data(), cells, items.size()});
            auto s4 = pam::diagnostics::scan(items, 0);
            std::printf("sgs tke: etime %g , e_mean %.9g , tke_min %.9g , tke_max %.9g , tk_max %.9g\n", etime_gcm,
                        s4[0].mean() / (s4[1].mean() + s4[2].mean()), s4[0].vmin[0], s4[0].vmax[0], s4[3].vmax[0]);
          }
          if (mods.sgs_horizontal) {                                         // the same scan: the greatest tk and tkh beside the cap they are
            const long long cells = (long long)crm_ny * crm_nx * nens * crm_nz;   // clipped at, kcap = 0.25 / (dt s), s = 1/dx^2 (+ 1/dy^2, ny > 1)
            std::vector<pam::diagnostics::Item> items;
            for (char const *n : {"tk", "tkh"}) items.push_back({n, 0, dm.get<real const, 4>(n).data(), cells, items.size()});
            auto s2 = pam::diagnostics::scan(items, 0);
            const double hdx = coupler.get_dx(), hdy = coupler.get_dy();
            const double hs = 1.0 / (hdx * hdx) + (crm_ny > 1 ? 1.0 / (hdy * hdy) : 0.0);
            std::printf("sgs horizontal: etime %g , kcap %.9g , tk_max %.9g , tkh_max %.9g\n", etime_gcm,
                        0.25 / (coupler.get_option<real>("crm_dt") * hs), s2[0].vmax[0], s2[1].vmax[0]);
          }
          if (mods.ls_forcing) {                                             // the same scan: the domain means of the winds, and temp of level 0
            const long long level = (long long)crm_ny * crm_nx * nens;
            std::vector<pam::diagnostics::Item> items;
            for (char const *n : {"uvel", "vvel"}) items.push_back({n, 0, dm.get<real const, 4>(n).data(), level * crm_nz, items.size()});
            items.push_back({"temp", 0, dm.get<real const, 4>("temp").data(), level, items.size()});
            auto s3 = pam::diagnostics::scan(items, 0);
            std::printf("ls forcing: etime %g , uvel %.9g , vvel %.9g , temp0 %.9g\n", etime_gcm, s3[0].mean(), s3[1].mean(), s3[2].mean());
          }
          if (mods.esmt) {                                                   // the level means of the scalars as they are now, averaged
            modules::esmt_detail::diagnose(coupler, "driver", nullptr, nullptr, false);
            const size_t n2 = (size_t)crm_nz * nens;
            std::vector<real> um(n2), vm(n2);
            if (hipMemcpy(um.data(), dm.get<real const, 2>("esmt_u_mean").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(vm.data(), dm.get<real const, 2>("esmt_v_mean").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess)
              endrun("memcpy");
            double su = 0, sv = 0;
            for (size_t c = 0; c < n2; c++) { su += um[c]; sv += vm[c]; }
            std::printf("esmt: etime %g , u_s %.9g , v_s %.9g , max_T_dt %.9g\n", etime_gcm, su / n2, sv / n2, esmt_max_t_dt);
          }
          if (mods.micro_ice) {                                              // the ice water path, the two rates, and the water budget
            fetch("cloud_ice");
            long double iwp = 0;
            const size_t level = (size_t)crm_ny * crm_nx * nens;
            for (int k = 0; k < crm_nz; k++) {
              long double row = 0;
              for (size_t c = 0; c < level; c++) row += buf[(size_t)k * level + c];
              iwp += row * (long double)(zint[k + 1] - zint[k]);
            }
            std::printf("micro ice: etime %g , iwp %.9g , precl %.9g , preci %.9g , water %.17g , water_start %.17g , precipitated %.17g\n", etime_gcm,
                        (double)(iwp / level), mean2d("precl"), mean2d("preci"), (double)micro_ice.compute_total_mass(coupler),
                        (double)ice_water_start, (double)ice_precip_sum);
          }
          char t[64];
          std::snprintf(t, sizeof(t), "%s%.6g", maxw_series.empty() ? "" : ",", maxw);
          maxw_series += t;
          num_out++;
          if (diag_out.is_open()) {
            std::vector<pam::diagnostics::Item> items;
            for (auto &n : diag_names) items.push_back({n, 0, dm.get<real const, 4>(n).data(), (long long)ncell, items.size()});
            auto whole = pam::diagnostics::scan(items, 0), members = pam::diagnostics::scan(items, nens);
            std::string o = "{\"crm_step\": " + std::to_string(crm_steps) + ", \"etime\": ";
            stats_json_number(o, etime_gcm);
            o += ", \"nens\": " + std::to_string(nens) + ", \"fields\": {";
            for (size_t f = 0; f < items.size(); f++) {
              o += (f ? ", \"" : "\"") + diag_names[f] + "\": {\"whole\": ";
              diag_json(o, whole[f]);
              o += ", \"members\": ";
              diag_json(o, members[f]);
              o += "}";
            }
            o += "}}\n";
            diag_out << o << std::flush;
            if (!diag_out) endrun("cannot write the --diag file");
          }
        }
        if (steps_limit > 0 && crm_steps >= steps_limit) stop = true;
      }
      if (clock.ceased()) accel_ceased_gcm_steps++;
      if (mods.vt) {                                                          // the GCM step's variances
        coupler.run_module("vt_compute_feedback", modules::vt_compute_feedback);
        std::string o = "{\"gcm_step\": " + std::to_string(step_gcm);
        std::vector<real> prof((size_t)crm_nz * nens);
        for (const char *what : {"var_start", "var", "feedback"}) {
          o += std::string(", \"") + what + "\": {";
          const char *q[3] = {"t", "q", "u"};
          for (int i = 0; i < (mods.vt_u ? 3 : 2); i++) {
            if (hipMemcpy(prof.data(), dm.get<real const, 2>(std::string("vt_") + what + "_" + q[i]).data(), prof.size() * sizeof(real),
                          hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
            o += std::string(i ? ", \"" : "\"") + q[i] + "\": [";
            for (size_t j = 0; j < prof.size(); j++) {
              if (j) o += ", ";
              stats_json_number(o, prof[j]);
            }
            o += "]";
          }
          o += "}";
        }
        o += "}\n";
        vt_out << o << std::flush;
        if (!vt_out) endrun("cannot write the --vt file");
      }
      if (coldiag_out.is_open()) {                                            // the GCM step's column diagnostics
        std::string o = "{\"gcm_step\": " + std::to_string(step_gcm) + ", \"crm_steps\": " + std::to_string(crm_steps_gcm) + ", \"nens\": " +
                        std::to_string(nens) + ", \"diagnostics\": {";
        bool first = true;
        for (const char *n : {"diag_cldtot", "diag_cldlow", "diag_cldmed", "diag_cldhgh", "diag_lwp", "diag_iwp", "diag_pw", "diag_precip_liq",
                              "diag_precip_ice"}) {
          if (!dm.entry_exists(n)) continue;
          o += std::string(first ? "\"" : ", \"") + n + "\": ";
          handoff_json_array(o, dm.get<real const, 1>(n).data(), {nens});
          first = false;
        }
        o += "}}\n";
        coldiag_out << o << std::flush;
        if (!coldiag_out) endrun("cannot write the --column-diag file");
      }
      if (fluxprof_out.is_open()) {                                           // the GCM step's flux profiles
        std::string o = "{\"gcm_step\": " + std::to_string(step_gcm) + ", \"crm_steps\": " + std::to_string(crm_steps_gcm) + ", \"nens\": " +
                        std::to_string(nens) + ", \"nz\": " + std::to_string(crm_nz) + ", \"profiles\": {";
        bool first = true;
        for (const char *n : {"prof_mcup", "prof_mcdn", "prof_mcuup", "prof_mcudn", "prof_cld", "prof_flux_t", "prof_flux_qt", "prof_flux_u",
                              "prof_flux_v", "prof_tke"}) {
          if (!dm.entry_exists(n)) continue;
          o += std::string(first ? "\"" : ", \"") + n + "\": ";
          handoff_json_array(o, dm.get<real const, 2>(n).data(), {crm_nz, nens});
          first = false;
        }
        o += "}}\n";
        fluxprof_out << o << std::flush;
        if (!fluxprof_out) endrun("cannot write the --flux-profiles file");
      }
      if (mods.handoff) {                                                     // the GCM step's aggregates and feedback
        coupler.run_module("compute_crm_feedback", modules::compute_crm_feedback);
        handoff_steps += std::string(handoff_steps.empty() ? "" : ", ") + "{\"gcm_step\": " + std::to_string(step_gcm) + ", \"crm_steps\": " +
                         std::to_string(crm_steps_gcm) + ", \"aggregates\": {";
        bool first = true;
        for (const char *n : {"rad_temperature", "rad_qv", "rad_qc", "rad_qi", "rad_cld"}) {
          if (!dm.entry_exists(n)) continue;
          handoff_steps += std::string(first ? "\"" : ", \"") + n + "\": ";
          handoff_json_array(handoff_steps, dm.get<real const, 4>(n).data(), {crm_nz, mods.handoff_rad_ny, mods.handoff_rad_nx, nens});
          first = false;
        }
        handoff_steps += "}, \"feedback\": {";
        first = true;
        for (const char *what : {"mean", "tend"})
          for (const char *q : {"t", "qv", "qc", "qi", "u", "v"}) {
            std::string n = std::string("crm_feedback_") + what + "_" + q;
            if (!dm.entry_exists(n)) continue;
            handoff_steps += std::string(first ? "\"" : ", \"") + what + "_" + q + "\": ";
            handoff_json_array(handoff_steps, dm.get<real const, 2>(n).data(), {crm_nz, nens});
            first = false;
          }
        handoff_steps += "}}";
      }
      if (stats) {                                                            // the GCM step's profiles
        coupler.run_module("horizontal_average", [&](pam::PamCoupler &c) { modules::horizontal_average(c, stat_havg); });
        char t[96];
        std::snprintf(t, sizeof(t), "%s{\"gcm_step\": %d, \"crm_steps\": %d, \"profiles\": {", stats_steps.empty() ? "" : ", ", step_gcm,
                      crm_steps_gcm);
        stats_steps += t;
        for (size_t f = 0; f < stat_names.size(); f++) {
          const int pnz = stat_names[f] == "precl" ? 1 : crm_nz;
          std::vector<real> prof((size_t)pnz * nens);
          if (hipMemcpy(prof.data(), dm.get<real const, 2>(stat_names[f] + "_time_average_horizontal_average").data(),
                        prof.size() * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
          stats_steps += (f ? ", \"" : "\"") + stat_names[f] + "\": [";
          for (int k = 0; k < pnz; k++) {
            stats_steps += k ? ", [" : "[";
            for (int e = 0; e < nens; e++) {
              if (e) stats_steps += ", ";
              stats_json_number(stats_steps, prof[(size_t)k * nens + e]);
            }
            stats_steps += "]";
          }
          stats_steps += "]";
        }
        stats_steps += "}}";
      }
    }
    if (stats) {
      std::string o = "{\"nens\": " + std::to_string(nens) + ", \"nz\": " + std::to_string(crm_nz) + ", \"crm_dt\": ";
      stats_json_number(o, dt_crm_phys);
      o += ", \"gcm_physics_dt\": ";
      stats_json_number(o, dt_gcm);
      o += ", \"fields\": [";
      for (size_t f = 0; f < stat_names.size(); f++) o += (f ? ", \"" : "\"") + stat_names[f] + "\"";
      o += "], \"gcm_steps\": [" + stats_steps + "]}\n";
      std::ofstream so(mods.stats);
      if (!so) endrun("cannot open the --stats file");
      so << o;
      if (!so) endrun("cannot write the --stats file");
    }
    if (mods.handoff) {
      std::string o = "{\"nens\": " + std::to_string(nens) + ", \"nz\": " + std::to_string(crm_nz) + ", \"rad_nx\": " +
                      std::to_string(mods.handoff_rad_nx) + ", \"rad_ny\": " + std::to_string(mods.handoff_rad_ny) + ", \"crm_dt\": ";
      stats_json_number(o, dt_crm_phys);
      o += ", \"gcm_physics_dt\": ";
      stats_json_number(o, dt_gcm);
      o += ", \"gcm_steps\": [" + handoff_steps + "]}\n";
      std::ofstream ho(mods.handoff_path);
      if (!ho) endrun("cannot open the --gcm-handoff file");
      ho << o;
      if (!ho) endrun("cannot write the --gcm-handoff file");
    }
    if (!mods.edges.empty()) {
      pam::VerticalInterp<5> vert_interp;
      vert_interp.init(dm.get<real const, 2>("vertical_interface_height"));
      real4d edges = vert_interp.cells_to_edges(dm.get<real const, 4>("temp"), vert_interp.BC_ZERO_GRADIENT, vert_interp.BC_ZERO_GRADIENT);
      std::vector<real> host(edges.size());
      if (hipMemcpy(host.data(), edges.data(), host.size() * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
      std::ofstream eo(mods.edges, std::ios::binary);
      if (!eo) endrun("cannot open the --edges file");
      eo.write((char *)host.data(), host.size() * sizeof(real));
      if (!eo) endrun("cannot write the --edges file");
    }
    if (hipDeviceSynchronize() != hipSuccess) endrun("device error");
    if (sf_in) (void)hipFree(sf_in);
    std::printf("Simulation Time: %g\n", etime_gcm);
    if (mods.surface_friction) {                                             // the fluxes an SGS scheme reads (--sgs-smag consumes them)
      const size_t n2 = (size_t)crm_ny * crm_nx * nens;
      std::vector<real> fu(n2), fv(n2), z0(nens);
      if (hipMemcpy(fu.data(), dm.get<real const, 3>("sfc_mom_flx_u").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(fv.data(), dm.get<real const, 3>("sfc_mom_flx_v").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(z0.data(), dm.get<real const, 1>("z0").data(), nens * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
      double fmax = 0, z0min = INFINITY, z0max = -INFINITY;
      bool ffin = true;
      for (size_t c = 0; c < n2; c++) {
        if (!std::isfinite(fu[c]) || !std::isfinite(fv[c])) ffin = false;
        fmax = std::max(fmax, std::max(std::fabs(fu[c]), std::fabs(fv[c])));
      }
      for (real z : z0) { z0min = std::min(z0min, (double)z); z0max = std::max(z0max, (double)z); }
      std::printf("surface friction: finite %s, max |sfc_mom_flx| %.9g, z0 [%.9g, %.9g]\n", ffin ? "true" : "false", fmax, z0min, z0max);
    }
    // statistics of the final state + the output file (same layout as the binary mode: the fields, then precl)
    std::vector<std::string> names = {"density_dry", "uvel", "vvel", "wvel", "temp"};
    for (auto &n : coupler.get_tracer_names()) names.push_back(n);
    std::ofstream out;
    if (outfile != "-") out.open(outfile, std::ios::binary);
    bool finite = true;
    double rho_min = INFINITY, t_min = INFINITY, t_max = -INFINITY, w_max = 0, qmin = INFINITY;
    long t_min_at = -1;
    for (size_t f = 0; f < names.size(); f++) {
      fetch(names[f]);
      for (size_t c = 0; c < ncell; c++) {
        const real v = buf[c];
        if (!std::isfinite(v)) finite = false;
        if (f == 0) rho_min = std::min(rho_min, (double)v);
        if (f == 3) w_max = std::max(w_max, (double)std::fabs(v));
        if (f == 4) { if (v < t_min) { t_min = v; t_min_at = (long)c; } t_max = std::max(t_max, (double)v); }
        if (f >= 5 && names[f].rfind("esmt_", 0) != 0) qmin = std::min(qmin, (double)v);      // (the scalars of --esmt carry a wind: either sign)
      }
      if (out.is_open()) out.write((char *)buf.data(), ncell * sizeof(real));
    }
    if (out.is_open()) {
      const size_t n2 = (size_t)crm_ny * crm_nx * nens;
      if (hipMemcpy(buf.data(), dm.get<real const, 3>("precl").data(), n2 * sizeof(real), hipMemcpyDeviceToHost) != hipSuccess) endrun("memcpy");
      out.write((char *)buf.data(), n2 * sizeof(real));
    }
#ifdef PAM_FUNCTION_TIMERS
    pam::function_timers::print();
#endif
    if (mods.sgs_moist || mods.sfc_fluxes)
      std::printf("{\"sgs_smag_moist\": %s, \"sgs_smag_surface_fluxes\": %s, \"sfc_shf\": %.17g, \"sfc_lhf\": %.17g}\n",
                  mods.sgs_moist ? "true" : "false", mods.sfc_fluxes ? "true" : "false", mods.sfc_shf, mods.sfc_lhf);
    if (mods.sgs_smag) std::printf("{\"sgs_smag_cs\": %.17g, \"sgs_smag_prandtl\": %.17g}\n", mods.sgs_cs, mods.sgs_prandtl);
    if (mods.sgs_tke) std::printf("{\"sgs_tke_cs\": %.17g, \"sgs_tke_ck\": %.17g}\n", mods.sgs_cs, mods.sgs_ck);
    if (mods.hyperdiff) std::printf("{\"hyperdiff_timescale\": %.17g}\n", mods.hyperdiff_tau);
    if (mods.accelerate)
      std::printf("{\"accel_factor\": %.9g, \"accel_uv\": %s, \"accel_max_ttend\": %.9g, \"accelerated_steps\": %d, \"ceased_gcm_steps\": %d}\n",
                  mods.accel_factor, mods.accel_uv ? "true" : "false", mods.accel_max_ttend, accel_steps, accel_ceased_gcm_steps);
    if (mods.vt)
      std::printf("{\"vt_rate\": %.17g, \"vt_u\": %s, \"vt_limit\": %.17g}\n", mods.vt_rate, mods.vt_u ? "true" : "false", mods.vt_limit);
    std::printf("{\"crm_steps\": %d, \"substeps\": %ld, \"etime\": %.9g, \"dt_crm_phys\": %.9g, \"nens\": %d, \"nx\": %d, \"ny\": %d, \"nz\": %d, "
                "\"finite\": %s, \"rho_d_min\": %.9g, \"temp_min\": %.9g, \"temp_max\": %.9g, \"maxw_final\": %.9g, \"maxw_any_output\": %.9g, "
                "\"temp_min_level\": %ld, \"tracer_min\": %.9g, \"maxw_series\": [%s], \"conservation_checked\": %s, \"conservation_violations\": %ld, "
                "\"conservation_max_rel_diff\": %.6e}\n",
                crm_steps, substeps, etime_gcm, dt_crm_phys, nens, crm_nx, crm_ny, crm_nz, finite ? "true" : "false", rho_min, t_min, t_max, w_max,
                maxw_all, t_min_at < 0 ? -1L : t_min_at / ((long)crm_ny * crm_nx * nens), qmin, maxw_series.c_str(), check ? "true" : "false", cons_violations, cons_max_rel);
    dycore.finalize(coupler);                                                // driver.cpp:285
  } catch (std::string &msg) {
    std::fprintf(stderr, "driver: endrun: %s\n", msg.c_str());
    rcode = 1;
  }
  return rcode;
}
#endif

int main(int argc, char **argv) {
  int gpus = 1, tile = 1, a = 1;
#ifndef PAMC_DYCORE
  if (argc >= 4 && std::string(argv[1]) == "--yaml") {
    int nens_override = 0, steps_limit = 0, b = 3;
    bool check = false;
    YamlDebug dbg;
    YamlModules mods;
    for (; b < argc - 1; b++) {
      const std::string o(argv[b]);
      if (o == "--nens" && b + 1 < argc - 1) nens_override = std::atoi(argv[++b]);
      else if (o == "--steps" && b + 1 < argc - 1) steps_limit = std::atoi(argv[++b]);
      else if (o == "--check") check = true;
      else if (o == "--no-micro") dbg.no_micro = true;
      else if (o == "--no-sponge") dbg.no_sponge = true;
      else if (o == "--sync") dbg.sync = true;
      else if (o == "--dump-init" && b + 1 < argc - 1) dbg.dump_init = argv[++b];
      else if (o == "--sat-adjust") mods.sat_adjust = true;
      else if (o == "--surface-friction" && b + 2 < argc - 1) {
        mods.surface_friction = true;
        mods.tau = std::atof(argv[++b]);
        mods.bflx = std::atof(argv[++b]);
      }
      else if (o == "--validate") mods.validate = true;
      else if (o == "--diag" && b + 1 < argc - 1) mods.diag = argv[++b];
      else if (o == "--stats" && b + 1 < argc - 1) mods.stats = argv[++b];
      else if (o == "--edges" && b + 1 < argc - 1) mods.edges = argv[++b];
      else if (o == "--radiation" && b + 3 < argc - 1) {
        mods.radiation = true;
        mods.rad_nx = std::atoi(argv[++b]);
        mods.rad_ny = std::atoi(argv[++b]);
        mods.rad_path = argv[++b];
      }
      else if (o == "--accelerate" && b + 1 < argc - 1) { mods.accelerate = true; mods.accel_factor = std::atof(argv[++b]); }
      else if (o == "--accel-uv") mods.accel_uv = true;
      else if (o == "--accel-max-ttend" && b + 1 < argc - 1) mods.accel_max_ttend = std::atof(argv[++b]);
      else if (o == "--vt" && b + 2 < argc - 1) { mods.vt = true; mods.vt_rate = std::atof(argv[++b]); mods.vt_path = argv[++b]; }
      else if (o == "--vt-u") mods.vt_u = true;
      else if (o == "--vt-limit" && b + 1 < argc - 1) mods.vt_limit = std::atof(argv[++b]);
      else if (o == "--hyperdiff" && b + 1 < argc - 1) { mods.hyperdiff = true; mods.hyperdiff_tau = std::atof(argv[++b]); }
      else if (o == "--sgs-smag" && b + 2 < argc - 1) { mods.sgs_smag = true; mods.sgs_cs = std::atof(argv[++b]); mods.sgs_prandtl = std::atof(argv[++b]); }
      else if (o == "--radiation-gray") {
        mods.radiation_gray = true;
        const std::string n(b + 1 < argc - 1 ? argv[b + 1] : "");                // the optional EVERY: an argument of digits only
        if (!n.empty() && n.find_first_not_of("0123456789") == std::string::npos) mods.radiation_gray_every = std::atoi(argv[++b]);
      }
      else if (o == "--shortwave" && b + 1 < argc - 1) {
        mods.shortwave = true;
        mods.sw_coszen = std::atof(argv[++b]);
        const std::string n(b + 1 < argc - 1 ? argv[b + 1] : "");                // the optional ALBEDO: an argument that is a number
        if (!n.empty() && n.find_first_not_of("0123456789.eE+") == std::string::npos) mods.sw_albedo = std::atof(argv[++b]);
      }
      else if (o == "--sgs-tke" && b + 2 < argc - 1) { mods.sgs_tke = true; mods.sgs_cs = std::atof(argv[++b]); mods.sgs_ck = std::atof(argv[++b]); }
      else if (o == "--sgs-horizontal") mods.sgs_horizontal = true;
      else if (o == "--sgs-moist") mods.sgs_moist = true;
      else if (o == "--micro-ice") mods.micro_ice = true;
      else if (o == "--sfc-fluxes" && b + 2 < argc - 1) { mods.sfc_fluxes = true; mods.sfc_shf = std::atof(argv[++b]); mods.sfc_lhf = std::atof(argv[++b]); }
      else if (o == "--surface" && b + 1 < argc - 1) {
        mods.surface = true;
        mods.surface_sst = std::atof(argv[++b]);
        const std::string n(b + 1 < argc - 1 ? argv[b + 1] : "");                // the optional DEPTH: an argument that is a number
        if (!n.empty() && n.find_first_not_of("0123456789.eE+") == std::string::npos) mods.surface_depth = std::atof(argv[++b]);
      }
      else if (o == "--ls-forcing" && b + 1 < argc - 1) { mods.ls_forcing = true; mods.ls_path = argv[++b]; }
      else if (o == "--coriolis" && b + 1 < argc - 1) { mods.coriolis = true; mods.ls_fcor = std::atof(argv[++b]); }
      else if (o == "--esmt") {
        mods.esmt = true;
        const std::string n(b + 1 < argc - 1 ? argv[b + 1] : "");                // the optional KMAX: an argument of digits only
        if (!n.empty() && n.find_first_not_of("0123456789") == std::string::npos) mods.esmt_kmax = std::atoi(argv[++b]);
      }
      else if (o == "--gcm-handoff" && b + 3 < argc - 1) {
        mods.handoff = true;
        mods.handoff_rad_nx = std::atoi(argv[++b]);
        mods.handoff_rad_ny = std::atoi(argv[++b]);
        mods.handoff_path = argv[++b];
      }
      else if (o == "--column-diag" && b + 1 < argc - 1) mods.column_diag = argv[++b];
      else if (o == "--flux-profiles" && b + 1 < argc - 1) mods.flux_profiles = argv[++b];
      else die("usage: driver --yaml <input.yaml> [--nens N] [--steps S] [--check] [--sat-adjust] [--surface-friction TAU BFLX] "
               "[--validate] [--diag PATH] [--stats PATH] [--edges PATH] [--radiation RAD_NX RAD_NY PATH] "
               "[--accelerate A [--accel-uv] [--accel-max-ttend X]] [--vt RATE PATH [--vt-u] [--vt-limit L]] [--hyperdiff TAU] [--sgs-smag CS PRANDTL] [--sgs-tke CS CK] [--sgs-horizontal] [--sgs-moist] [--sfc-fluxes SHF LHF] [--surface SST [DEPTH]] [--ls-forcing PATH [--coriolis F]] [--esmt [KMAX]] [--radiation-gray [EVERY]] [--shortwave COSZEN [ALBEDO]] [--micro-ice] "
               "[--gcm-handoff RAD_NX RAD_NY PATH] [--column-diag PATH] [--flux-profiles PATH] <output.bin | ->");
    }
    if (mods.radiation_gray && mods.radiation) die("--radiation-gray and --radiation both fill the one radiation slot: give one of them");
    if (mods.radiation_gray && mods.radiation_gray_every < 1) die("--radiation-gray EVERY must be >= 1");
    if (mods.shortwave && !mods.radiation_gray) die("--shortwave COSZEN [ALBEDO] needs --radiation-gray [EVERY]: the sun belongs to the native scheme");
    if (mods.sgs_smag && mods.sgs_tke) die("--sgs-smag and --sgs-tke both stand in the SGS slot: give one of them");
    if (mods.sgs_tke && (!(mods.sgs_cs > 0) || !(mods.sgs_ck > 0))) die("--sgs-tke CS CK needs CS > 0 and CK > 0");
    if ((mods.sgs_moist || mods.sfc_fluxes) && !mods.sgs_smag && !mods.sgs_tke) die("--sgs-moist and --sfc-fluxes need --sgs-smag CS PRANDTL or --sgs-tke CS CK");
    if (mods.sgs_horizontal && !mods.sgs_smag && !mods.sgs_tke) die("--sgs-horizontal needs --sgs-smag CS PRANDTL or --sgs-tke CS CK: it mixes with the closure's tk and tkh");
    if (mods.surface && !mods.sgs_smag && !mods.sgs_tke) die("--surface SST [DEPTH] needs --sgs-smag CS PRANDTL or --sgs-tke CS CK: the closure is what takes the fluxes up");
    if (mods.coriolis && !mods.ls_forcing) die("--coriolis F needs --ls-forcing PATH with the rows ug and vg: the force acts about a geostrophic wind");
    if (mods.surface && mods.sfc_fluxes) die("--surface and --sfc-fluxes both fill sfc_shf and sfc_lhf: give one of them");
    if (mods.surface && (!(mods.surface_sst > 0) || mods.surface_depth < 0)) die("--surface SST [DEPTH] needs SST > 0 K and DEPTH >= 0 m");
    return run_yaml(argv[2], nens_override, steps_limit, check, argv[argc - 1], dbg, mods);
  }
#endif
  Job J;
  for (; a < argc && argv[a][0] == '-' && argv[a][1] == '-'; a++) {
    const std::string o(argv[a]);
    if (o == "--gpus" && a + 1 < argc) gpus = std::atoi(argv[++a]);
    else if (o == "--tile" && a + 1 < argc) tile = std::atoi(argv[++a]);
    else if (o == "--bench" && a + 2 < argc) { J.bench_steps = std::atoi(argv[++a]); J.bench_warmup = std::atoi(argv[++a]); }
    else if (o == "--accelerate" && a + 1 < argc) { J.accelerate = true; J.accel_factor = std::atof(argv[++a]); }
    else if (o == "--accel-uv") J.accel_uv = true;
    else if (o == "--accel-max-ttend" && a + 1 < argc) J.accel_max_ttend = std::atof(argv[++a]);
    else if (o == "--vt" && a + 1 < argc) { J.vt = true; J.vt_rate = std::atof(argv[++a]); }
    else if (o == "--vt-u") J.vt_u = true;
    else if (o == "--vt-limit" && a + 1 < argc) J.vt_limit = std::atof(argv[++a]);
    else if (o == "--hyperdiff" && a + 1 < argc) { J.hyperdiff = true; J.hyperdiff_tau = std::atof(argv[++a]); }
    else die("usage: driver [--gpus N] [--tile R] [--bench K W] [--accelerate A [--accel-uv] [--accel-max-ttend X]] [--vt RATE [--vt-u] [--vt-limit L]] [--hyperdiff TAU] <input.bin> <output.bin>");
  }
  if (argc - a != 2 || gpus < 1 || tile < 1)
    die("usage: driver [--gpus N] [--tile R] [--bench K W] [--accelerate A [--accel-uv] [--accel-max-ttend X]] [--vt RATE [--vt-u] [--vt-limit L]] [--hyperdiff TAU] <input.bin> <output.bin>");
  std::ifstream in(argv[a], std::ios::binary);
  if (!in) die("cannot open input");
  int64_t hdr[8];
  in.read((char *)hdr, sizeof(hdr));
  const int nens_in = hdr[0];
  J.nens = nens_in * tile; J.nx = hdr[1]; J.ny = hdr[2]; J.nz = hdr[3]; J.nt = hdr[4]; J.nsteps = hdr[5];
  J.mode_a = (hdr[6] & 1) != 0; J.with_sponge = (hdr[6] & 2) != 0; J.with_micro = (hdr[6] & 4) != 0;
  J.halo_roundtrip = (hdr[6] & 8) != 0; J.has_consts = hdr[7] != 0;
  if (J.with_micro && J.nt != 3) die("the Kessler microphysics registers exactly 3 tracers");
  in.read((char *)J.geo, sizeof(J.geo));
  in.read((char *)J.consts, sizeof(J.consts));
  J.zint.resize(J.nz + 1);
  in.read((char *)J.zint.data(), J.zint.size() * sizeof(real));
  J.flags.resize(2 * J.nt);
  in.read((char *)J.flags.data(), J.flags.size());
  in.read((char *)&J.idWV, sizeof(J.idWV));
  const size_t ncol = (size_t)J.nz * J.ny * J.nx;
  J.nens_in = nens_in;
  J.raw.assign(5 + J.nt, std::vector<real>(ncol * nens_in));
  for (int f = 0; f < 5 + J.nt; f++) {
    in.read((char *)J.raw[f].data(), J.raw[f].size() * sizeof(real));
    if (!in) die("short input file");
  }
  J.want_output = std::string(argv[a + 1]) != "-";        // "-": no output file (bench runs of large ensembles)
  if (J.want_output) {
    J.fields.assign(5 + J.nt, std::vector<real>(ncol * J.nens));
    J.precl.assign((size_t)J.ny * J.nx * J.nens, 0.0);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) die("no HIP device");
  HostMin hmin(gpus);
  std::vector<BenchResult> bench(gpus);
  std::vector<std::string> errors(gpus);
  std::string name;
  std::vector<std::thread> threads;
  for (int r = 0; r < gpus; r++)
    threads.emplace_back([&, r]() {
      try {
        run_rank(J, r, gpus, ndev, hmin, bench[r], name);
      } catch (std::string &msg) {
        errors[r] = msg.empty() ? "endrun" : msg;
        hmin.fail();
      }
    });
  for (auto &t : threads) t.join();
  for (int r = 0; r < gpus; r++)
    if (!errors[r].empty()) { std::fprintf(stderr, "driver: rank %d: endrun: %s\n", r, errors[r].c_str()); return 1; }
  std::printf("Dycore: %s\n", name.c_str());
  if (J.accelerate && J.bench_steps == 0)
    std::printf("{\"accel_factor\": %.9g, \"crm_steps\": %d, \"ceased\": %s}\n", J.accel_factor, J.accel_crm_steps, J.accel_ceased ? "true" : "false");
  if (J.bench_steps > 0) {
    double sec = 0;
    for (auto &b : bench) sec = std::max(sec, b.seconds);
    std::printf("{\"launcher\": \"cpp\", \"ranks\": %d, \"devices\": %d, \"nens_total\": %d, \"nx\": %d, \"ny\": %d, \"nz\": %d, "
                "\"num_tracers\": %d, \"steps\": %d, \"warmup\": %d, \"seconds\": %.9g, \"substeps\": %ld}\n",
                gpus, ndev, J.nens, J.nx, J.ny, J.nz, J.nt, J.bench_steps, J.bench_warmup, sec, bench[0].substeps);
  }
  if (J.want_output) {
    std::ofstream out(argv[a + 1], std::ios::binary);
    for (auto &f : J.fields) out.write((char *)f.data(), f.size() * sizeof(real));
    if (J.with_micro) out.write((char *)J.precl.data(), J.precl.size() * sizeof(real));
  }
  return 0;
}
