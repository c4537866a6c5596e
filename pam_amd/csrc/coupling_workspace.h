// coupling_workspace.h -- where the arrays of a coupling layer's workspace lie (the SHOC and the P3 layer of modules_kernels.hip, contract in
// include/pam_amd_modules.h).  Host arithmetic only, no HIP: tests/cxx/coupling_layout.cpp checks it without a GPU.  This layout decides
// what memory a handed-in shoc_main / p3_main may write.
#pragma once
#include "../../include/pam_amd_modules.h"

namespace pama {
namespace coupling {
constexpr int GUARD = 8;   // doubles of canary before the first array, between any two and after the last
inline long long round8(long long n) { return (n + 7) / 8 * 8; }

// an array that has no element: KEEP_SLOT gives it a slot of its own (a non-null pointer nothing may be written through: SHOC's
// wtracer_sfc and qtracers without tracers), NO_SLOT gives it none and a null pointer (P3's p3_tend_out without tendency planes)
enum class ZeroSize { KEEP_SLOT, NO_SLOT };

// offset[i] = where array i of size[i] doubles begins, in doubles from the base of the allocation, or -1 for an array without a slot;
// returns the doubles of the whole allocation.  Every slot is rounded up to a multiple of 8 doubles
inline long long carve(const long long *size, int n, int guard, ZeroSize policy, long long *offset) {
  long long at = guard;
  for (int i = 0; i < n; i++) {
    const bool slot = size[i] > 0 || policy == ZeroSize::KEEP_SLOT;
    offset[i] = slot ? at : -1;
    if (slot) at += round8(size[i]) + guard;
  }
  return at;
}

// how many elements an array has: N columns, Z levels, T tracers (SHOC) or tendency planes (P3)
enum Extent { COLUMN, CELL, INTERFACE, COMPONENT_CELL, TRACER_CELL, TRACER_COLUMN, THREE_COLUMN };
inline long long count(Extent e, long long N, long long Z, long long T) {
  switch (e) {
    case COLUMN: return N;
    case CELL: return Z * N;
    case INTERFACE: return (Z + 1) * N;
    case COMPONENT_CELL: return 2 * Z * N;   // hwind: u_wind, v_wind
    case TRACER_CELL: return T * Z * N;
    case TRACER_COLUMN: return T * N;
    default: return 3 * N;                   // col_location
  }
}

// one array of a layer: its pointer in the args struct and its extent.  A table holds them in the order of the allocation
template <class ARGS> struct Array { double *ARGS::*ptr; Extent extent; };
using ShocArray = Array<pam_amd_shoc_args_t>;
using P3Array = Array<pam_amd_p3_args_t>;

constexpr int SHOC_NARRAYS = 46, P3_NARRAYS = 43;
#define ROW(name, extent) {&pam_amd_shoc_args_t::name, extent}
constexpr ShocArray SHOC_TABLE[SHOC_NARRAYS] = {
    ROW(host_dx, COLUMN), ROW(host_dy, COLUMN), ROW(thv, CELL), ROW(zt_grid, CELL), ROW(zi_grid, INTERFACE), ROW(pres, CELL), ROW(presi, INTERFACE),
    ROW(pdel, CELL), ROW(wthl_sfc, COLUMN), ROW(wqw_sfc, COLUMN), ROW(uw_sfc, COLUMN), ROW(vw_sfc, COLUMN), ROW(wtracer_sfc, TRACER_COLUMN),
    ROW(w_field, CELL), ROW(inv_exner, CELL), ROW(phis, COLUMN), ROW(host_dse, CELL), ROW(tke, CELL), ROW(thetal, CELL), ROW(qw, CELL),
    ROW(hwind, COMPONENT_CELL), ROW(qtracers, TRACER_CELL), ROW(wthv_sec, CELL), ROW(tk, CELL), ROW(ql, CELL), ROW(cldfrac, CELL), ROW(pblh, COLUMN),
    ROW(ustar, COLUMN), ROW(obklen, COLUMN), ROW(mix, CELL), ROW(isotropy, CELL), ROW(w_sec, CELL), ROW(thl_sec, INTERFACE), ROW(qw_sec, INTERFACE),
    ROW(qwthl_sec, INTERFACE), ROW(wthl_sec, INTERFACE), ROW(wqw_sec, INTERFACE), ROW(wtke_sec, INTERFACE), ROW(uw_sec, INTERFACE),
    ROW(vw_sec, INTERFACE), ROW(w3, INTERFACE), ROW(wqls_sec, CELL), ROW(brunt, CELL), ROW(ql2, CELL), ROW(tkh, CELL), ROW(exner, CELL)};
#undef ROW
#define ROW(name, extent) {&pam_amd_p3_args_t::name, extent}
constexpr P3Array P3_TABLE[P3_NARRAYS] = {
    ROW(qc, CELL), ROW(nc, CELL), ROW(qr, CELL), ROW(nr, CELL), ROW(th_atm, CELL), ROW(qv, CELL), ROW(qi, CELL), ROW(qm, CELL), ROW(ni, CELL), ROW(bm, CELL),
    ROW(pres, CELL), ROW(dz, CELL), ROW(nc_nuceat_tend, CELL), ROW(nccn_prescribed, CELL), ROW(ni_activated, CELL), ROW(inv_qc_relvar, CELL),
    ROW(precip_liq_surf, COLUMN), ROW(precip_ice_surf, COLUMN), ROW(diag_eff_radius_qc, CELL), ROW(diag_eff_radius_qi, CELL),
    ROW(diag_eff_radius_qr, CELL), ROW(bulk_qi, CELL), ROW(precip_total_tend, CELL), ROW(nevapr, CELL), ROW(qr_evap_tend, CELL), ROW(dpres, CELL),
    ROW(inv_exner, CELL), ROW(qv2qi_depos_tend, CELL), ROW(precip_liq_flux, INTERFACE), ROW(precip_ice_flux, INTERFACE), ROW(cld_frac_r, CELL),
    ROW(cld_frac_l, CELL), ROW(cld_frac_i, CELL), ROW(p3_tend_out, TRACER_CELL), ROW(mu_c, CELL), ROW(lamc, CELL), ROW(liq_ice_exchange, CELL),
    ROW(vap_liq_exchange, CELL), ROW(vap_ice_exchange, CELL), ROW(q_prev, CELL), ROW(t_prev, CELL), ROW(col_location, THREE_COLUMN), ROW(exner, CELL)};
#undef ROW

// the layout of a whole table: offset[i] of row i (or -1), returns the doubles of the allocation
template <class ARGS, int NA>
long long carve_table(const Array<ARGS> (&table)[NA], long long N, long long Z, long long T, ZeroSize policy, long long (&offset)[NA]) {
  long long size[NA];
  for (int i = 0; i < NA; i++) size[i] = count(table[i].extent, N, Z, T);
  return carve(size, NA, GUARD, policy, offset);
}
// a row's pointer may be null exactly where carve gives the row no slot
template <class ARGS> bool may_be_null(const Array<ARGS> &row, long long N, long long Z, long long T, ZeroSize policy) {
  return policy == ZeroSize::NO_SLOT && count(row.extent, N, Z, T) == 0;
}
constexpr ZeroSize SHOC_ZERO_SIZE = ZeroSize::KEEP_SLOT, P3_ZERO_SIZE = ZeroSize::NO_SLOT;
}  // namespace coupling
}  // namespace pama
