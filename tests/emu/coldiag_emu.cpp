// coldiag_emu.cpp -- HOST EMULATION of the CRM column diagnostics kernels (pam_amd/csrc/coldiag_device.h, compiled with g++
// -ffp-contract=off).  TEST INFRASTRUCTURE ONLY (never shipped, never linked into libpam_amd_awfl.so).  The loops mirror the two kernels of
// modules_kernels.hip; the bits must depend neither on the order of the scan's threads nor on which walkers hold the 16 slots of a member:
//   scan_order  0  the (column, member) threads in ascending order, the kernel's unroll factor        (coldiag_scan_kernel)
//               1  the same threads in descending order
//               2  ascending, four levels' loads together where the kernel has SCAN_UNROLL: the order of the arithmetic does not depend on the unroll factor
//   mapping     1  block slots: 16 walkers per member, one slot each; the slot sums go to an array laid out like the kernel's LDS (rows of 64
//                  members, blocks of `me` consecutive members) and are folded in ascending slot order   (coldiag_mean_block_kernel)
//               2  thread slots: one walker takes the 16 slots one after the other                       (coldiag_mean_thread_kernel)
//               3  four walkers of four slots each, every one folding onto what the one before it handed on
#include <cstddef>
#include <vector>

#include "../../pam_amd/csrc/coldiag_device.h"

using namespace pama::coldiag;
namespace rd = pama::rad;

namespace {
// the mean of one column array for every member -> tot[e]
void column_means(int nens, int ncol, const double *in, int mapping, int me, std::vector<double> &tot) {
  const long long stride = nens, rowstride = (long long)ncol * nens;
  const double r = r_columns(ncol);
  if (mapping == 1) {
    std::vector<double> red((size_t)NS * 64);
    for (int b = 0; b * me < nens; b++) {
      for (int slot = 0; slot < NS; slot++)
        for (int m = 0; m < me; m++) {
          const int e = b * me + m;
          double acc[1] = {0.0};
          if (e < nens) {
            const double *f[1] = {in + e};
            rd::slot_walk<Means>(f, stride, rowstride, ncol, ncol, slot, rd::Cursor{slot / ncol, slot % ncol}, r, acc);
          }
          red[(size_t)slot * 64 + m] = acc[0];
        }
      for (int m = 0; m < me && b * me + m < nens; m++) tot[b * me + m] = pama::msa::fold(&red[m], 64);
    }
    return;
  }
  const int walkers = mapping == 2 ? 1 : 4, each = NS / walkers;
  for (int e = 0; e < nens; e++) {
    const double *f[1] = {in + e};
    double t[1] = {0.0};
    for (int w = 0; w < walkers; w++) rd::slots_walk<Means>(f, stride, rowstride, ncol, ncol, w * each, each, r, t);
    tot[e] = t[0];
  }
}

}  // namespace

extern "C" {

// fields[6], zint, precip[2] or null, out[9] as pam_amd_column_diagnostics has them, in host memory
int emu_column_diagnostics(int nens, int nx, int ny, int nz, const double *const *fields, const double *zint, const double *const *precip, double R_d,
                           double R_v, double p_low, double p_high, double cwp_threshold, double *const *out, double factor, int scan_order,
                           int mapping, int me) {
  if (scan_order < 0 || scan_order > 2 || mapping < 1 || mapping > 3 || me < 1 || me > 64) return -1;
  const int ncol = nx * ny;
  const long long level = (long long)ncol * nens;
  const Params P{R_d, R_v, p_low, p_high, cwp_threshold};
  const double *f[NF];
  for (int i = 0; i < NF; i++) f[i] = fields[i];
  // the workspace: an array for every column value that has an output
  std::vector<std::vector<double>> store(NW);
  double *ws[NW];
  for (int q = 0; q < NW; q++) {
    if (out[q]) store[q].assign((size_t)level, -7.0);
    ws[q] = out[q] ? store[q].data() : nullptr;
  }
  for (long long n = 0; n < level; n++) {
    const long long t = scan_order == 1 ? level - 1 - n : n;
    Column c;
    if (scan_order == 2) column_scan<4>(f, zint, t, level, nens, (int)(t % nens), nz, P, c);
    else column_scan<SCAN_UNROLL>(f, zint, t, level, nens, (int)(t % nens), nz, P, c);
    column_store(c, ws, t, P);
  }
  std::vector<double> tot((size_t)nens);
  for (int q = 0; q < NO; q++) {
    const double *in = q < NW ? ws[q] : (precip ? precip[q - NW] : nullptr);
    if (!in) continue;
    column_means(nens, ncol, in, mapping, me, tot);
    for (int e = 0; e < nens; e++) out[q][e] = rd::accumulate(out[q][e], tot[e], factor);
  }
  return 0;
}

}
