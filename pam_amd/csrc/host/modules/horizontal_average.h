// modules/horizontal_average.h -- modules::horizontal_average(coupler, var_list) with the reference's signature
// (pam_core/modules/horizontal_average.h:25), forwarding to pam_amd_horizontal_average (include/pam_amd_modules.h).
// Registers "<var>_horizontal_average" {nz,nens} as the reference does and sums in its serial order.  Deliberate deviations (the
// reference does not compile): the last dimension is checked against the coupler's nens; an output that exists
// already is reused (a second call overwrites it); a rank of 5 or more is an error; the whole list is validated before anything is
// registered or written.
#pragma once
#include <string>
#include <tuple>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace modules {

inline void horizontal_average(pam::PamCoupler &coupler, std::vector<std::tuple<std::string, bool>> var_list) {
  int nens = coupler.get_nens();
  auto &dm = coupler.get_data_manager_device_readwrite();
  int num_vars = var_list.size();
  std::vector<int> nzs(num_vars), ncols(num_vars);
  for (int i = 0; i < num_vars; i++) {                                        // :43-62, every entry before any registration
    auto var_name = std::get<0>(var_list[i]);
    auto has_vertical_dim = std::get<1>(var_list[i]);
    auto havg_name = var_name + std::string("_horizontal_average");
    auto shape = dm.get_shape(var_name);
    int r = shape.size();
    if (shape[r - 1] != nens) endrun("ERROR: Last dimension must be nens (" + var_name + ")");
    long long ncol = 0;
    if (has_vertical_dim) {
      if (r == 1) endrun("ERROR: Cannot horizontally average a 1-D variable (" + var_name + ")");
      if (r == 2) endrun("ERROR: Cannot horizontally average a nz,nens variable (" + var_name + ")");
      if (r == 3) { nzs[i] = shape[0];   ncol = shape[1]; }
      if (r == 4) { nzs[i] = shape[0];   ncol = (long long)shape[1] * shape[2]; }
      if (r >= 5) endrun("ERROR: Only two horizontal dimensions allowed (" + var_name + ")");
    } else {
      if (r == 1) endrun("ERROR: Cannot horizontally average a 1-D variable (" + var_name + ")");
      if (r == 2) { nzs[i] = 1;   ncol = shape[0]; }
      if (r == 3) { nzs[i] = 1;   ncol = (long long)shape[0] * shape[1]; }
      if (r >= 4) endrun("ERROR: Only two horizontal dimensions allowed (" + var_name + ")");
    }
    if (ncol < 1 || ncol > 0x7fffffffLL) endrun("ERROR: horizontal_average: bad number of columns (" + var_name + ")");
    ncols[i] = (int)ncol;
    if (dm.entry_exists(havg_name) && dm.get_shape(havg_name) != std::vector<int>{nzs[i], nens})
      endrun("ERROR: " + havg_name + " exists with a shape other than {nz,nens}");
  }
  if (num_vars == 0) return;
  std::vector<double const *> in(num_vars);
  std::vector<double *> out(num_vars);
  for (int i = 0; i < num_vars; i++) {
    auto var_name = std::get<0>(var_list[i]);
    auto havg_name = var_name + std::string("_horizontal_average");
    if (!dm.entry_exists(havg_name)) dm.register_and_allocate<real>(havg_name, "", {nzs[i], nens});
    in[i] = dm.get_collapsed<real const>(var_name).data();
    out[i] = dm.get<real, 2>(havg_name).data();
  }
  int rc = pam_amd_horizontal_average(nens, num_vars, nzs.data(), ncols.data(), in.data(), out.data(), nullptr);
  if (rc) endrun(pam_amd_awfl_last_error());
}

}  // namespace modules
