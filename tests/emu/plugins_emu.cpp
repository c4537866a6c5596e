// plugins_emu.cpp -- HOST EMULATION of the arithmetic of the forced radiation plug-in and the coupler's pressure array
// (pam_amd/csrc/plugins_device.h, compiled with g++ -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into
// libpam_amd_awfl.so).  The loops mirror the kernels of modules_kernels.hip: one update per cell, the rad cell found per row.
#include "../../pam_amd/csrc/plugins_device.h"

using namespace pama::plugins;

extern "C" {

// temp: (nz,ny,nx,nens) in/out; tend: (nz,rad_ny,rad_nx,nens)
void emu_radiation_forced(int nens, int nx, int ny, int nz, int rad_nx, int rad_ny, double *temp, const double *tend, double cp_d,
                          double dt) {
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        const long long row = ((long long)k * ny + j) * nx + i;
        const long long rad = ((long long)k * rad_ny + rad_index(j, ny, rad_ny)) * rad_nx + rad_index(i, nx, rad_nx);
        for (int e = 0; e < nens; e++) temp[row * nens + e] = radiation_forced(temp[row * nens + e], tend[rad * nens + e], cp_d, dt);
      }
}

void emu_compute_pressure(long long n, const double *rho_d, const double *rho_v, const double *temp, double R_d, double R_v,
                          double *pressure) {
  for (long long i = 0; i < n; i++) pressure[i] = compute_pressure(rho_d[i], rho_v[i], temp[i], R_d, R_v);
}

}
