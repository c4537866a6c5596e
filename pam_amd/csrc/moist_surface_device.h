// moist_surface_device.h -- per-cell arithmetic of two coupler modules, as __host__ __device__ functions: the HIP kernels in
// modules_kernels.hip call them, and tests/emu/moist_surface_emu.cpp compiles the same bodies with g++ (-ffp-contract=off).
//   saturation adjustment   pam_core/modules/saturation_adjustment.h:8-113
//   surface friction        pam_core/modules/surface_friction.h:16-63 (z0_est, diag_ustar) and the per-cell flux of :107-167
// Every expression keeps the reference's operation order; contraction into fma is switched off inside each body, so the device
// results differ from the host's only where the device library's exp / log / atan differ from glibc's (last place).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PAMA_MS_HD __host__ __device__ __forceinline__
#else
#define PAMA_MS_HD inline
#endif

#if defined(__clang__)
#define PAMA_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PAMA_NO_CONTRACT
#endif

namespace pama {
namespace moist {

// saturation_adjustment.h:33 (absolute tolerance on the bisection bracket) and the iteration cap.  The reference's loop has no cap;
// its bracket halves down to 1e-6 within 54 iterations wherever it converges at all, and only shrinks by one ulp per step (~1045
// iterations from the largest double) otherwise.  It never ends on rho_v = inf (the bracket becomes inf / NaN) or on absurd
// magnitudes where the midpoint stalls one ulp away from a bound wider than tol.  2048 never binds where the reference terminates;
// a capped cell keeps the state of its last iteration.
constexpr double SATADJ_TOL = 1.e-6;
constexpr int SATADJ_MAX_ITER = 2048;
constexpr double SATADJ_CP_L = 4188.0;   // saturation_adjustment.h:141

// yakl::max (a > b ? a : b) and std::min / std::max ((b < a) ? b : a, (a < b) ? b : a): the reference uses both
PAMA_MS_HD double yakl_max_(double a, double b) { return a > b ? a : b; }
PAMA_MS_HD double std_min_(double a, double b) { return (b < a) ? b : a; }
PAMA_MS_HD double std_max_(double a, double b) { return (a < b) ? b : a; }

PAMA_MS_HD double saturation_vapor_pressure(double temp) {            // :9-12
  PAMA_NO_CONTRACT
  const double tc = temp - 273.15;
  return 610.94 * exp(17.625 * tc / (243.04 + tc));
}

PAMA_MS_HD double latent_heat_condensation(double temp) {             // :15-18
  PAMA_NO_CONTRACT
  const double tc = temp - 273.15;
  return (2500.8 - 2.36 * tc + 0.0016 * tc * tc - 0.00006 * tc * tc * tc) * 1000;
}

PAMA_MS_HD double cp_moist(double rho_d, double rho_v, double rho_c, double cp_d, double cp_v, double cp_l) {   // :21-25
  PAMA_NO_CONTRACT
  const double rho = rho_d + rho_v + rho_c;
  return rho_d / rho * cp_d + rho_v / rho * cp_v + rho_c / rho * cp_l;
}

// compute_adjusted_state (:28-113).  Returns the iterations taken: 0 when the cell is in neither branch (rho_v, rho_c, temp are left
// as they are -- NaN states among them); otherwise they hold the adjusted state.
PAMA_MS_HD int compute_adjusted_state(double rho, double rho_d, double &rho_v, double &rho_c, double &temp, double R_v, double cp_d,
                                   double cp_v, double cp_l) {
  PAMA_NO_CONTRACT
  const double svp = saturation_vapor_pressure(temp);
  const double pv = rho_v * R_v * temp;
  const bool cond = pv > svp;
  if (!cond && !(pv < svp && rho_c > 0)) return 0;
  // condensation (:42-74): x moves vapour to cloud; evaporation (:77-111): x moves cloud to vapour.  Same bisection, mirrored signs.
  double x1 = 0, x2 = cond ? rho_v : rho_c;
  const double Lv = latent_heat_condensation(temp);                 // at the INCOMING temperature, every iteration (:55, :92)
  double rv_loc = rho_v, rc_loc = rho_c, temp_loc = temp;
  int it = 0;
  while (it < SATADJ_MAX_ITER) {
    it++;
    const double x = (x1 + x2) / 2;
    if (cond) {
      rv_loc = yakl_max_(0., rho_v - x);
      rc_loc = yakl_max_(0., rho_c + x);
    } else {
      rv_loc = yakl_max_(0., rho_v + x);
      rc_loc = yakl_max_(0., rho_c - x);
    }
    const double cp = cp_moist(rho_d, rv_loc, rc_loc, cp_d, cp_v, cp_l);
    temp_loc = cond ? temp + x * Lv / (rho * cp) : temp - x * Lv / (rho * cp);
    const double svp_loc = saturation_vapor_pressure(temp_loc);
    const double pv_loc = rv_loc * R_v * temp_loc;
    // still super- (sub-) saturated: move more, otherwise less
    if (cond ? (pv_loc > svp_loc) : (pv_loc < svp_loc)) x1 = x;
    else x2 = x;
    if (fabs(x2 - x1) <= SATADJ_TOL) break;
  }
  rho_v = rv_loc;
  rho_c = rc_loc;
  temp = temp_loc;
  return it;
}

// surface_friction.h:8-12
constexpr double SF_VONK = 0.4;
constexpr double SF_EPS = 1.0e-10;
constexpr double SF_AM = 4.8;
constexpr double SF_BM = 19.3;
constexpr double SF_PI = 3.14159;    // the reference's literal, not M_PI

// z0_est (:16-31): roughness height for momentum
PAMA_MS_HD double z0_est(double z, double bflx, double wnd, double ustar) {
  PAMA_NO_CONTRACT
  const double c1 = SF_PI / 2.0 - 3.0 * log(2.0);
  const double rlmo = -bflx * SF_VONK / (ustar * ustar * ustar + SF_EPS);
  const double zeta = std_min_(1.0, z * rlmo);
  double psi1;
  if (zeta >= 0.0) {
    psi1 = -SF_AM * zeta;
  } else {
    const double x = sqrt(sqrt(1.0 - SF_BM * zeta));
    psi1 = 2.0 * log(1.0 + x) + log(1.0 + x * x) - 2.0 * atan(x) + c1;
  }
  const double lnz = std_max_(0.0, SF_VONK * wnd / (ustar + SF_EPS) + psi1);
  return z * exp(-lnz);
}

// diag_ustar (:44-63): friction speed; exactly 8 iterations, and only when bflx != 0.  Note zeta > 0 here, zeta >= 0 in z0_est.
PAMA_MS_HD double diag_ustar(double z, double bflx, double wnd, double z0) {
  PAMA_NO_CONTRACT
  const double lnz = log(z / z0);
  const double klnz = SF_VONK / lnz;
  const double c1 = SF_PI / 2.0 - 3.0 * log(2.0);
  double ustar = wnd * klnz;
  if (bflx != 0.0) {
    for (int iterate = 0; iterate < 8; iterate++) {
      const double rlmo = -bflx * SF_VONK / (ustar * ustar * ustar + SF_EPS);
      const double zeta = std_min_(1.0, z * rlmo);
      if (zeta > 0.0) {
        ustar = SF_VONK * wnd / (lnz + SF_AM * zeta);
      } else {
        const double x = sqrt(sqrt(1.0 - SF_BM * zeta));
        const double psi1 = 2.0 * log(1.0 + x) + log(1.0 + x * x) - 2.0 * atan(x) + c1;
        ustar = wnd * SF_VONK / (lnz - psi1);
      }
    }
  }
  return ustar;
}

// surface_friction_init, per member (:96-103): z0 from the GCM's lowest-level wind and the horizontal-mean surface density
PAMA_MS_HD double surface_friction_z0(double zmid0, double bflx, double gcm_u0, double gcm_v0, double tau, double rho_horz_mean) {
  PAMA_NO_CONTRACT
  const double wnd_spd = std_max_(1.0, sqrt(gcm_u0 * gcm_u0 + gcm_v0 * gcm_v0));
  const double ustar = sqrt(tau / rho_horz_mean);
  const double z0 = z0_est(zmid0, bflx, wnd_spd, ustar);
  return std_max_(0.00001, std_min_(1.0, z0));
}

// compute_surface_friction, per cell (:147-166): the surface momentum flux in SHOC's units [m2/s2].  rho_mid{0,1,2}: rho_d + rho_v
// of the cell's lowest three levels; dz = zint(1) - zint(0)
PAMA_MS_HD void surface_friction_cell(double u, double v, double u_mean, double v_mean, double rho_mean, double zmid0, double bflx,
                                   double z0, double rho_mid0, double rho_mid1, double rho_mid2, double dz, double &flx_u,
                                   double &flx_v) {
  PAMA_NO_CONTRACT
  const double u2 = u * u;
  const double v2 = v * v;
  const double wnd_spd = std_max_(1.0, sqrt(u2 + v2));
  const double ustar = diag_ustar(zmid0, bflx, wnd_spd, z0);
  const double tau00 = rho_mean * ustar * ustar;
  const double fu = -(u - u_mean) / wnd_spd * tau00;
  const double fv = -(v - v_mean) / wnd_spd * tau00;
  const double rho_int0 = (rho_mid0 + rho_mid1) / 2;
  const double rho_int1 = (rho_mid1 + rho_mid2) / 2;
  const double rho_sfc = 2.0 * rho_int0 - rho_int1;
  flx_u = fu * rho_sfc / dz;
  flx_v = fv * rho_sfc / dz;
}

}  // namespace moist
}  // namespace pama
