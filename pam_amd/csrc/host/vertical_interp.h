// vertical_interp.h -- pam::VerticalInterp<ord> with the reference's members (pam_core/vertical_interp.h): hs, BC_ZERO_GRADIENT,
// BC_ZERO_VALUE, init(zint), cells_to_edges(data, bc_lower, bc_upper); forwards to pam_amd_vertical_interp_* (include/
// pam_amd_modules.h).  Orders 3 and 5 only: the reference's sample_val for orders 7 and 9 drops a `* z`.
//
// OWNERSHIP.  The reference returns a freshly allocated, reference-counted real4d.  The work-alike's arrays are non-owning views
// (pam_coupler.h), so THIS OBJECT owns the storage of the returned edges: it is allocated on the first call, reused by every later
// call of the same shape (the earlier result is overwritten), replaced when the shape changes, and freed with the object.  A caller
// that needs two results at once copies the first, or uses two objects.  The work runs on the default stream, unsynchronised, like the
// module adaptors.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pam_coupler.h"
#include "pam_amd_awfl.h"
#include "pam_amd_modules.h"

namespace pam {

template <unsigned int ord>
class VerticalInterp {
  static_assert(ord == 3 || ord == 5, "pam::VerticalInterp: orders 3 and 5 only (the reference's orders 7 and 9 do not interpolate)");
 public:
  int  static constexpr hs = (ord-1)/2;
  real static constexpr eps = 1.0e-20;

  int static constexpr BC_ZERO_GRADIENT = 0;
  int static constexpr BC_ZERO_VALUE    = 1;

  VerticalInterp() {}
  VerticalInterp(VerticalInterp const &) = delete;
  VerticalInterp &operator=(VerticalInterp const &) = delete;
  ~VerticalInterp() { release(); }

  // zint: DEVICE (nz+1,nens).  May be called again with another grid.
  inline void init( realConst2d zint ) {
    release();
    if (zint.dims().size() != 2) endrun("ERROR: VerticalInterp::init: zint must be (nz+1,nens)");
    int rc = pam_amd_vertical_interp_init(ord, zint.extent(0) - 1, zint.extent(1), zint.data(), nullptr, &handle);
    if (rc) endrun(pam_amd_awfl_last_error());
    nz = zint.extent(0) - 1;
    nens = zint.extent(1);
  }

  // data: DEVICE (nz,ny,nx,nens) -> DEVICE (nz+1,ny,nx,nens), owned by this object and reused between calls of the same shape
  inline real4d cells_to_edges( realConst4d data , int bc_lower , int bc_upper ) const {
    if (!handle) endrun("ERROR: VerticalInterp::cells_to_edges called before init");
    if (data.dims().size() != 4) endrun("ERROR: VerticalInterp::cells_to_edges: data must be (nz,ny,nx,nens)");
    if (data.extent(0) != nz || data.extent(3) != nens) endrun("ERROR: VerticalInterp::cells_to_edges: data does not have init's nz and nens");
    std::vector<int> dims = {data.extent(0) + 1, data.extent(1), data.extent(2), data.extent(3)};
    if (dims != edge_dims) {
      if (edge_store) (void)hipFree(edge_store);
      edge_store = nullptr;
      edge_dims.clear();
      size_t n = 1;
      for (int d : dims) n *= (size_t)(d > 0 ? d : 0);
      if (n == 0) endrun("ERROR: VerticalInterp::cells_to_edges: empty array");
      if (hipMalloc((void **)&edge_store, n * sizeof(real)) != hipSuccess) endrun("ERROR: device allocation failed for the edges");
      edge_dims = dims;
    }
    int rc = pam_amd_vertical_interp_cells_to_edges(handle, data.extent(1), data.extent(2), data.data(), bc_lower, bc_upper, edge_store,
                                                    nullptr);
    if (rc) endrun(pam_amd_awfl_last_error());
    return real4d(edge_store, edge_dims);
  }

 private:
  void release() {
    if (handle) (void)pam_amd_vertical_interp_finalize(handle);
    handle = nullptr;
    if (edge_store) (void)hipFree(edge_store);
    edge_store = nullptr;
    edge_dims.clear();
  }

  void *handle = nullptr;
  int nz = 0, nens = 0;
  mutable real *edge_store = nullptr;
  mutable std::vector<int> edge_dims;
};

}  // namespace pam
