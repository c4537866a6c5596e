"""Coupler modules around the dycore in the CRM step loop, mirroring `namespace modules` of pam_core/modules/
(free functions taking the coupler).  Arithmetic is in libpam_amd_awfl.so (pam_amd/csrc/modules_kernels.hip)."""
import ctypes as C

import torch

from . import capi
from .capi import check


def sponge_layer(coupler):
    """modules::sponge_layer(coupler)  (pam_core/modules/sponge_layer.h:8-95).  Options read exactly as the
    reference: "sponge_num_layers" (default 5), "sponge_time_scale" (default 60), "crm_dt"."""
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    num_layers = coupler.get_option("sponge_num_layers") if coupler.option_exists("sponge_num_layers") else 5
    time_scale = coupler.get_option("sponge_time_scale") if coupler.option_exists("sponge_time_scale") else 60.0
    dm = coupler.get_data_manager_device_readwrite()
    names = ["density_dry", "uvel", "vvel", "wvel", "temp"] + coupler.get_tracer_names()
    tens = [dm.get(n) for n in names]
    zint = dm.get("vertical_interface_height", readonly=True)
    zmid = dm.get("vertical_midpoint_height", readonly=True)
    ptrs = (C.c_void_p * len(tens))(*[t.data_ptr() for t in tens])
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_sponge_layer(nens, nx, ny, nz, len(tens), ptrs, zint.data_ptr(), zmid.data_ptr(),
                                       float(coupler.get_option("crm_dt")), int(num_layers), float(time_scale),
                                       None, torch.cuda.current_stream(coupler.device).cuda_stream))


GCM_FORCING_CRM = ("density_dry", "uvel", "vvel", "temp", "water_vapor", "cloud_water", "ice", "cloud_water_num", "ice_num",
                   "rain_num")
GCM_FORCING_GCM = ("gcm_density_dry", "gcm_uvel", "gcm_vvel", "gcm_temp", "gcm_water_vapor", "gcm_cloud_water", "gcm_cloud_ice",
                   "gcm_num_liq", "gcm_num_ice", "gcm_num_rain")
GCM_FORCING_TEND = (("rho_d", "dry density"), ("uvel", "u-velocity"), ("vvel", "v-velocity"), ("temp", "temperature"),
                    ("qtot", "tot water mix ratio"), ("qv", "vap water mix ratio"), ("ql", "liq water mix ratio"),
                    ("qi", "ice water mix ratio"), ("rho_v", "water vapor density"), ("rho_l", "cloud water density"),
                    ("rho_i", "cloud ice density"), ("nc", "liq number"), ("ni", "ice number"), ("nr", "rain number"))


def _ptr_table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def compute_gcm_forcing_tendencies(coupler):
    """modules::compute_gcm_forcing_tendencies(coupler)  (pam_core/modules/gcm_forcing.h:17-210): once per GCM step.
    Reads option "gcm_physics_dt"; registers the 14 "gcm_forcing_tend_*" (nz,nens) entries on first use (:132-147)."""
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    crm = [dm.get(n, readonly=True) for n in GCM_FORCING_CRM]
    gcm = [dm.get(n, readonly=True) for n in GCM_FORCING_GCM[:7]] + [dm.get(n) for n in GCM_FORCING_GCM[7:]]   # :51-53 non-const
    if not dm.entry_exists("gcm_forcing_tend_uvel"):
        for n, d in GCM_FORCING_TEND:
            dm.register_and_allocate("gcm_forcing_tend_" + n, "GCM forcing for " + d, (nz, nens), ("z", "nens"))
    tend = [dm.get("gcm_forcing_tend_" + n) for n, _ in GCM_FORCING_TEND]
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_gcm_forcing_compute(nens, nx, ny, nz, _ptr_table(crm), _ptr_table(gcm), _ptr_table(tend),
                                              float(coupler.get_option("gcm_physics_dt")),
                                              torch.cuda.current_stream(coupler.device).cuda_stream))


def apply_gcm_forcing_tendencies(coupler):
    """modules::apply_gcm_forcing_tendencies(coupler)  (gcm_forcing.h:297-440): every CRM step.  Options "crm_dt",
    "gcm_physics_dt".  Returns the hole-filling mask (bit s: species s filled; bit 4+s: whole-CRM fallback)."""
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    crm = [dm.get(n) for n in GCM_FORCING_CRM]
    gcm = [dm.get(n, readonly=True) for n in GCM_FORCING_GCM]
    tend = [dm.get("gcm_forcing_tend_" + n, readonly=n not in ("rho_v", "rho_l", "rho_i")) for n, _ in GCM_FORCING_TEND]
    dz = dm.get("vertical_cell_dz")
    work = torch.empty(6 * nz * nens + 2 * nens + 4, dtype=torch.float64, device=coupler.device)
    mask = C.c_int()
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_gcm_forcing_apply(nens, nx, ny, nz, _ptr_table(crm), _ptr_table(gcm), _ptr_table(tend), dz.data_ptr(),
                                            float(coupler.get_option("crm_dt")), float(coupler.get_option("gcm_physics_dt")),
                                            work.data_ptr(), torch.cuda.current_stream(coupler.device).cuda_stream,
                                            C.byref(mask)))
    return mask.value   # the call synchronised the stream, so `work` may be dropped


BROADCAST_GCM = ("gcm_density_dry", "gcm_uvel", "gcm_vvel", "gcm_wvel", "gcm_temp", "gcm_water_vapor")
BROADCAST_CRM = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor")


def _broadcast(coupler, n):
    lib = capi.load()
    dm = coupler.get_data_manager_device_readwrite()
    gcm = [dm.get(name, readonly=True) for name in BROADCAST_GCM[:n]]
    crm = [dm.get(name) for name in BROADCAST_CRM[:n]]
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_broadcast_initial_gcm_column(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), n,
                                                       _ptr_table(gcm), _ptr_table(crm),
                                                       torch.cuda.current_stream(coupler.device).cuda_stream))


def broadcast_initial_gcm_column(coupler):
    """modules::broadcast_initial_gcm_column(coupler)  (pam_core/modules/broadcast_initial_gcm_column.h:8-41)."""
    _broadcast(coupler, 6)


def broadcast_initial_gcm_column_dry_density(coupler):
    """modules::broadcast_initial_gcm_column_dry_density(coupler)  (broadcast_initial_gcm_column.h:44-62)."""
    _broadcast(coupler, 1)


def perturb_temperature(coupler, ids, magnitude=0.1):
    """modules::perturb_temperature(coupler, id, magnitude)  (pam_core/modules/perturb_temperature.h:10-63); `ids` is one
    integer per member.  splitmix64 stands in for the reference's yakl::Random (see include/pam_amd_modules.h)."""
    lib = capi.load()
    nens = coupler.get_nens()
    ids = torch.as_tensor(ids, dtype=torch.int32, device=coupler.device).contiguous()
    if ids.numel() != nens:
        from .coupler import endrun
        endrun("ERROR: size of id array must be the same as nens")        # perturb_temperature.h:20
    temp = coupler.get_data_manager_device_readwrite().get("temp")
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_perturb_temperature(nens, coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), temp.data_ptr(),
                                              ids.data_ptr(), float(magnitude),
                                              torch.cuda.current_stream(coupler.device).cuda_stream))
    return ids   # keeps the id array alive until the caller drops it (the launch is asynchronous)


def supercell_init(vert_interface, R_d, R_v, grav):
    """supercell_init(...) of the standalone driver (standalone/mmf_simplified/supercell_init.h:7-135) on the device:
    vert_interface (nz+1,) CUDA tensor -> (rho_d_col, uvel_col, vvel_col, wvel_col, temp_col, rho_v_col), each (nz,)."""
    lib = capi.load()
    z = vert_interface.contiguous()
    if z.dim() != 1 or z.dtype != torch.float64 or not z.is_cuda:
        from .coupler import endrun
        endrun("ERROR: supercell_init: vert_interface must be a 1-D fp64 device array")
    nz = z.numel() - 1
    cols = [torch.empty(nz, dtype=torch.float64, device=z.device) for _ in range(6)]
    with torch.cuda.device(z.device):
        check(lib.pam_amd_supercell_init(nz, z.data_ptr(), float(R_d), float(R_v), float(grav), *[c.data_ptr() for c in cols],
                                         torch.cuda.current_stream(z.device).cuda_stream))
    return tuple(cols)


SATURATION_CONDENSATE = {"kessler": "cloud_liquid", "p3": "cloud_water", "ice1m": "cloud_liquid"}     # saturation_adjustment.h:126-129


def saturation_adjustment(coupler):
    """modules::saturation_adjustment(coupler)  (pam_core/modules/saturation_adjustment.h:116-147): condenses super-saturation,
    evaporates cloud towards saturation.  Options "micro" (kessler | p3), "R_v", "cp_d", "cp_v"; cp_l = 4188."""
    from .coupler import endrun
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    rho_d, temp, rho_v = dm.get("density_dry"), dm.get("temp"), dm.get("water_vapor")
    micro = coupler.get_option("micro")
    if micro not in SATURATION_CONDENSATE:
        endrun("ERROR: saturation_adjustment.h only currently supports kessler and p3 microphysics")
    rho_c = dm.get(SATURATION_CONDENSATE[micro])
    massy = [dm.get(n) for n in coupler.get_tracer_names() if coupler.get_tracer_info(n)[3]]    # :130-137, registration order
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_saturation_adjustment(nens, nx, ny, nz, rho_d.data_ptr(), rho_v.data_ptr(), rho_c.data_ptr(), temp.data_ptr(),
                                                len(massy), _ptr_table(massy), float(coupler.get_option("R_v")),
                                                float(coupler.get_option("cp_d")), float(coupler.get_option("cp_v")), 4188.0,
                                                torch.cuda.current_stream(coupler.device).cuda_stream))


def _member_array(coupler, x, what):
    from .coupler import endrun
    nens = coupler.get_nens()
    t = torch.as_tensor(x, dtype=torch.float64, device=coupler.device).contiguous()
    if t.dim() != 1 or t.numel() != nens:
        endrun("ERROR: surface_friction_init: %s needs nens values" % what)
    return t


def surface_friction_init(coupler, tau, bflx):
    """modules::surface_friction_init(coupler, tau_in, bflx_in)  (pam_core/modules/surface_friction.h:66-104); tau, bflx: one value
    per member.  Registers "z0" and "sfc_bflx" (nens) as the reference does, and "sfc_mom_flx_u/v" (ny,nx,nens) when no SGS scheme
    has (SHOC registers them in PAM, SGS.h:119-120)."""
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    tau, bflx = _member_array(coupler, tau, "tau"), _member_array(coupler, bflx, "bflx")
    dm = coupler.get_data_manager_device_readwrite()
    dm.register_and_allocate("z0", "Momentum roughness height [m]", (nens,), ("nens",))
    dm.register_and_allocate("sfc_bflx", "large-scale sfc buoyancy flux [K m/s]", (nens,), ("nens",))
    for n in ("sfc_mom_flx_u", "sfc_mom_flx_v"):
        if not dm.entry_exists(n):
            dm.register_and_allocate(n, "surface momentum flux", (ny, nx, nens), ("y", "x", "nens"))
    args = [dm.get(n) for n in ("density_dry", "water_vapor", "vertical_midpoint_height", "gcm_uvel", "gcm_vvel")]
    args += [tau, bflx] + [dm.get(n) for n in ("z0", "sfc_bflx", "sfc_mom_flx_u", "sfc_mom_flx_v")]
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_surface_friction_init(nens, nx, ny, nz, *[a.data_ptr() for a in args],
                                                torch.cuda.current_stream(coupler.device).cuda_stream))
    return tau, bflx   # keep the inputs alive until the caller drops them (the launch is asynchronous)


def compute_surface_friction(coupler):
    """modules::compute_surface_friction(coupler)  (pam_core/modules/surface_friction.h:107-167): "sfc_mom_flx_u/v" from the
    level-0 winds, the roughness height and buoyancy flux of the init, in [m2/s2]."""
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    args = [dm.get(n, readonly=True) for n in ("density_dry", "water_vapor", "uvel", "vvel", "vertical_midpoint_height",
                                                 "vertical_interface_height")]
    args += [dm.get(n) for n in ("z0", "sfc_bflx", "sfc_mom_flx_u", "sfc_mom_flx_v")]
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_surface_friction_compute(nens, nx, ny, nz, *[a.data_ptr() for a in args],
                                                   torch.cuda.current_stream(coupler.device).cuda_stream))


def _stats_collapse(dm, name, has_vertical_dim, nens):
    """(nz, ncol) of a variable as horizontal_average.h:43-62 reads it; endrun on every shape the reference rejects, and (deviations,
    DESIGN.md section 8) on a last dimension other than the coupler's nens and on a rank of 5 or more"""
    from .coupler import endrun
    shape = dm.get_shape(name)
    r = len(shape)
    if shape[-1] != nens:
        endrun("ERROR: Last dimension must be nens (%s)" % name)
    if r == 1:
        endrun("ERROR: Cannot horizontally average a 1-D variable (%s)" % name)
    if has_vertical_dim:
        if r == 2:
            endrun("ERROR: Cannot horizontally average a nz,nens variable (%s)" % name)
        if r > 4:
            endrun("ERROR: Only two horizontal dimensions allowed (%s)" % name)
        nz, ncol = shape[0], (shape[1] if r == 3 else shape[1] * shape[2])
    else:
        if r > 3:
            endrun("ERROR: Only two horizontal dimensions allowed (%s)" % name)
        nz, ncol = 1, (shape[0] if r == 2 else shape[0] * shape[1])
    if ncol > 0x7fffffff:
        endrun("ERROR: horizontal_average: bad number of columns (%s)" % name)
    return nz, ncol


def horizontal_average(coupler, var_list):
    """modules::horizontal_average(coupler, var_list)  (pam_core/modules/horizontal_average.h:25-75): var_list holds (name,
    has_vertical_dim) pairs; registers "<name>_horizontal_average" (nz,nens) -- or reuses it: a second call overwrites it -- and
    sets it to the mean over the columns, summed serially in ascending column order as the reference does.  The whole list is
    validated before anything is registered or written."""
    from .coupler import endrun
    lib = capi.load()
    nens = coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    items = []
    for name, has_vertical_dim in var_list:
        nz, ncol = _stats_collapse(dm, name, bool(has_vertical_dim), nens)
        havg = name + "_horizontal_average"
        if dm.entry_exists(havg) and dm.get_shape(havg) != [nz, nens]:
            endrun("ERROR: %s exists with a shape other than {nz,nens}" % havg)
        items.append((name, havg, nz, ncol))
    if not items:
        return
    for name, havg, nz, _ in items:
        if not dm.entry_exists(havg):
            dm.register_and_allocate(havg, "", (nz, nens))
    ins = [dm.get_collapsed(n, readonly=True) for n, _, _, _ in items]
    outs = [dm.get(h) for _, h, _, _ in items]
    nzs = (C.c_int * len(items))(*[it[2] for it in items])
    ncols = (C.c_int * len(items))(*[it[3] for it in items])
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_horizontal_average(nens, len(items), nzs, ncols, _ptr_table(ins), _ptr_table(outs),
                                             torch.cuda.current_stream(coupler.device).cuda_stream))


def _sizes(shapes):
    import math
    return (C.c_longlong * len(shapes))(*[math.prod(s) for s in shapes])


def time_average_init(coupler, names):
    """modules::time_average_init(coupler, names)  (pam_core/modules/time_average.h:8-36): registers "<name>_time_average" with the
    variable's own shape -- or reuses it -- and zeroes it (once per GCM step).  The whole list is validated first."""
    from .coupler import endrun
    lib = capi.load()
    dm = coupler.get_data_manager_device_readwrite()
    names = list(names)
    shapes = []
    for name in names:
        shape = dm.get_shape(name)
        tavg = name + "_time_average"
        if dm.entry_exists(tavg) and dm.get_shape(tavg) != shape:
            endrun("ERROR: %s exists with a shape other than %s's" % (tavg, name))
        shapes.append(shape)
    if not names:
        return
    for name, shape in zip(names, shapes):
        if not dm.entry_exists(name + "_time_average"):
            dm.register_and_allocate(name + "_time_average", "", tuple(shape))
    tavg = [dm.get_collapsed(n + "_time_average") for n in names]
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_time_average_zero(len(names), _sizes(shapes), _ptr_table(tavg),
                                            torch.cuda.current_stream(coupler.device).cuda_stream))


def time_average_accumulate(coupler, names, weight=1):
    """modules::time_average_accumulate(coupler, names)  (time_average.h:39-72; every CRM step): "<name>_time_average" +=
    name * (crm_dt / gcm_physics_dt), element by element.  Options "crm_dt", "gcm_physics_dt" (> 0).  The whole list is validated
    first: a name without its time average (no init) raises and nothing is written.  weight: how many steps of model time this CRM
    step counts (MsaClock under mean-state acceleration); it multiplies the factor, and 1 leaves it as it is."""
    import math
    from .coupler import endrun
    lib = capi.load()
    crm_dt = float(coupler.get_option("crm_dt"))
    gcm_dt = float(coupler.get_option("gcm_physics_dt"))
    if not gcm_dt > 0:
        endrun("ERROR: time_average_accumulate: gcm_physics_dt must be positive")
    factor = crm_dt / gcm_dt * float(weight)
    if not math.isfinite(factor):
        endrun("ERROR: time_average_accumulate: crm_dt / gcm_physics_dt x weight is not finite")
    dm = coupler.get_data_manager_device_readwrite()
    names = list(names)
    shapes = []
    for name in names:
        shape = dm.get_shape(name)
        tavg = name + "_time_average"
        if not dm.entry_exists(tavg):
            endrun("ERROR: %s does not exist: call time_average_init first" % tavg)
        if dm.get_shape(tavg) != shape:
            endrun("ERROR: %s has a shape other than %s's" % (tavg, name))
        shapes.append(shape)
    if not names:
        return
    var = [dm.get_collapsed(n, readonly=True) for n in names]
    tavg = [dm.get_collapsed(n + "_time_average") for n in names]
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_time_average_accumulate(len(names), _sizes(shapes), _ptr_table(var), _ptr_table(tavg), factor,
                                                  torch.cuda.current_stream(coupler.device).cuda_stream))


VALIDATE_KINDS = {torch.float64: 0, torch.float32: 1, torch.int32: 2, torch.int64: 3}


def validate_fields(tensors, positive):
    """The state check of DataManager::validate / validate_all (pam_core/DataManager.h:408-509) as one device scan
    (pam_amd_validate_fields): `tensors` is a list of contiguous float64, float32, int32 or int64 tensors on one device (a view offset
    by some elements is fine), `positive` one flag per tensor (positive-definite: negative values are offenders).  Returns
    (count, first), int64 numpy arrays of shape (len(tensors), 3): per tensor the number of NaNs, of infinities (either sign) and of
    negative values, and the lowest flat index of each (-1 where the count is 0).  Reads only; launched on the current stream, which
    is synchronised once."""
    import numpy as np
    from .coupler import endrun
    tensors, positive = list(tensors), [bool(p) for p in positive]
    if len(tensors) != len(positive):
        endrun("ERROR: validate_fields: one positive flag per tensor")
    count = np.zeros((len(tensors), 3), dtype=np.int64)
    first = np.full((len(tensors), 3), -1, dtype=np.int64)
    if not tensors:
        return count, first
    for t in tensors:
        if t.dtype not in VALIDATE_KINDS:
            endrun("ERROR: validate_fields: dtype %s is not float64, float32, int32 or int64" % t.dtype)
        if not t.is_contiguous():
            endrun("ERROR: validate_fields: contiguous tensors only")
        if t.numel() < 1:
            endrun("ERROR: validate_fields: empty tensor")
        if t.device != tensors[0].device:
            endrun("ERROR: validate_fields: the tensors must live on one device")
    n = len(tensors)
    kinds = (C.c_int * n)(*[VALIDATE_KINDS[t.dtype] for t in tensors])
    sizes = (C.c_longlong * n)(*[t.numel() for t in tensors])
    pos = (C.c_int * n)(*[int(p) for p in positive])
    device = tensors[0].device
    with torch.cuda.device(device):
        check(capi.load().pam_amd_validate_fields(n, kinds, sizes, _ptr_table(tensors), pos,
                                                  count.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                  first.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                  torch.cuda.current_stream(device).cuda_stream))
    return count, first


DIAGNOSTIC_KINDS = {torch.float64: 0, torch.float32: 1}


def field_diagnostics(tensors, members=0):
    """What the fields look like, as one device scan (pam_amd_field_diagnostics; the reference's DEBUG_PRINT_SUM / AVG / MIN / MAX,
    pam_core/pam_const.h:308-333): `tensors` is a list of contiguous float64 or float32 tensors on one device (a view offset by some
    elements is fine).  members = 0: one result per tensor; members = M >= 1: one per ensemble member, the member being the fastest
    axis (numel % M == 0).  Returns a dict of numpy arrays of shape (len(tensors),) or (len(tensors), M): "vmin", "vmax" (float64, the
    extreme element's own bits; NaNs take no part, +inf / -inf where every element is one), "argmin", "argmax" (int64 flat indices into
    the tensor, the lowest among equal values, -1 where every element is a NaN), "nan_count" (int64) and "vsum" (float64, the sum by
    the fixed tree of include/pam_amd_modules.h: the same bits from run to run and under member chunking).  max|x| is
    max(-vmin, vmax), the mean vsum / n.  Reads only; launched on the current stream, which is synchronised once."""
    import numpy as np
    from .coupler import endrun
    tensors, members = list(tensors), int(members)
    if members < 0:
        endrun("ERROR: field_diagnostics: members must be >= 0")
    shape = (len(tensors),) if members == 0 else (len(tensors), members)
    out = {k: np.zeros(shape, dtype=np.float64) for k in ("vmin", "vmax", "vsum")}
    out.update({k: np.zeros(shape, dtype=np.int64) for k in ("argmin", "argmax", "nan_count")})
    if not tensors:
        return out
    for t in tensors:
        if t.dtype not in DIAGNOSTIC_KINDS:
            endrun("ERROR: field_diagnostics: dtype %s is not float64 or float32" % t.dtype)
        if not t.is_contiguous():
            endrun("ERROR: field_diagnostics: contiguous tensors only")
        if t.numel() < 1:
            endrun("ERROR: field_diagnostics: empty tensor")
        if t.numel() % max(members, 1):
            endrun("ERROR: field_diagnostics: the number of elements must be a multiple of members")
        if t.device != tensors[0].device:
            endrun("ERROR: field_diagnostics: the tensors must live on one device")
    n = len(tensors)
    kinds = (C.c_int * n)(*[DIAGNOSTIC_KINDS[t.dtype] for t in tensors])
    sizes = (C.c_longlong * n)(*[t.numel() for t in tensors])
    device = tensors[0].device
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    with torch.cuda.device(device):
        check(capi.load().pam_amd_field_diagnostics(n, kinds, sizes, _ptr_table(tensors), members,
                                                    out["vmin"].ctypes.data_as(dp), out["vmax"].ctypes.data_as(dp),
                                                    out["vsum"].ctypes.data_as(dp), out["argmin"].ctypes.data_as(lp),
                                                    out["argmax"].ctypes.data_as(lp), out["nan_count"].ctypes.data_as(lp),
                                                    torch.cuda.current_stream(device).cuda_stream))
    return out


# ---- CRM mean-state acceleration (Jones, Bretherton and Pritchard 2015; E3SM-MMF's crm_accel_factor, crm_accel_uv).  Not part of the
# reference tree: the contract is this project's (include/pam_amd_modules.h; numpy restatement: tests/msa_ref.py)
MSA_CONDENSATE = {"kessler": ("cloud_liquid", None), "p3": ("cloud_water", "ice"), "none": (None, None),
                  "ice1m": ("cloud_liquid", "cloud_ice")}
MSA_QUANTITIES = ("t", "q", "u", "v")


class MsaClock:
    """The step clock of an accelerated CRM loop (the twin of modules::MsaClock).  nstop: unaccelerated CRM steps per GCM step;
    1 + accel_factor must be an integer that divides it (as E3SM requires), otherwise the constructor raises.  A step that was
    accelerated counts 1 + accel_factor steps of model time; the step that raised the cease flag counts 1, and so does every later step
    of the GCM step.  The count is an integer and cannot overshoot nstop; advance() returns the step's weight in
    time_average_accumulate."""

    def __init__(self, nstop, accel_factor):
        import math
        from .coupler import endrun
        if int(nstop) != nstop or nstop < 1:
            endrun("ERROR: mean-state acceleration: nstop must be >= 1")
        a = float(accel_factor)
        if not (a >= 0) or not math.isfinite(a):
            endrun("ERROR: mean-state acceleration: crm_accel_factor must be finite and >= 0")
        steps = 1 + a
        if steps != math.floor(steps) or steps > nstop or int(nstop) % int(steps) != 0:
            endrun("ERROR: mean-state acceleration: 1 + crm_accel_factor must be an integer that divides the number of CRM steps")
        self.nstop, self.per_step, self.count, self.ceased = int(nstop), int(steps), 0, False

    def done(self):
        return self.count >= self.nstop

    def accelerating(self):
        """does the next step run msa_diagnose / msa_accelerate?"""
        return not self.ceased and self.per_step > 1

    def advance(self, cease):
        """closes a CRM step; cease: what msa_accelerate returned (False for a step that did not call it)"""
        if cease:
            self.ceased = True
        weight = self.per_step if self.accelerating() else 1
        self.count += weight
        return weight


def _msa_arrays(coupler):
    from .coupler import endrun
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("accel_ceaseflag"):
        endrun("ERROR: mean-state acceleration: call msa_init first")
    micro = coupler.get_option("micro") if coupler.option_exists("micro") else "none"
    if micro not in MSA_CONDENSATE:
        endrun("ERROR: mean-state acceleration only knows the kessler, p3 and none microphysics")
    cloud, ice = MSA_CONDENSATE[micro]
    fields = [dm.get("temp"), dm.get("water_vapor"), dm.get(cloud, readonly=True) if cloud else None,
              dm.get(ice, readonly=True) if ice else None, dm.get("uvel"), dm.get("vvel")]
    save = [dm.get("accel_save_" + q) for q in MSA_QUANTITIES]
    tend = [dm.get("accel_tend_" + q) for q in MSA_QUANTITIES]
    return fields, save, tend, dm.get("accel_ceaseflag")


def _msa_table(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def msa_init(coupler):
    """First in every GCM step: registers "accel_save_{t,q,u,v}", "accel_tend_{t,q,u,v}" (nz,nens) and the cease word "accel_ceaseflag"
    (int32) on first use, zeroes the word and sets option "crm_accel_ceaseflag" = False.  Options: "crm_accel_factor" (>= 0, required),
    "crm_accel_uv" (default False), "crm_accel_max_ttend" (default 5 K)."""
    import math
    from .coupler import endrun
    if not coupler.option_exists("crm_accel_factor"):
        endrun("ERROR: mean-state acceleration: option crm_accel_factor is not set")
    a = float(coupler.get_option("crm_accel_factor"))
    if not (a >= 0) or not math.isfinite(a):
        endrun("ERROR: mean-state acceleration: crm_accel_factor must be finite and >= 0")
    if not coupler.option_exists("crm_accel_uv"):
        coupler.set_option("crm_accel_uv", False)
    if not coupler.option_exists("crm_accel_max_ttend"):
        coupler.set_option("crm_accel_max_ttend", 5.0)
    if not float(coupler.get_option("crm_accel_max_ttend")) > 0:
        endrun("ERROR: mean-state acceleration: crm_accel_max_ttend must be positive")
    nz, nens = coupler.get_nz(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("accel_ceaseflag"):
        for q in MSA_QUANTITIES:
            dm.register_and_allocate("accel_save_" + q, "level mean at the start of the CRM step", (nz, nens), ("z", "nens"))
            dm.register_and_allocate("accel_tend_" + q, "change of the level mean over the CRM step", (nz, nens), ("z", "nens"))
        dm.register_and_allocate("accel_ceaseflag", "mean-state acceleration ceased in this GCM step", (1,), dtype=torch.int32)
    dm.get("accel_ceaseflag").zero_()
    coupler.set_option("crm_accel_ceaseflag", False)


def msa_diagnose(coupler):
    """First in a CRM step, before GCM forcing: saves the level means of temp, total water (water_vapor + cloud + ice, by option
    "micro"), uvel and vvel.  Writes nothing else."""
    lib = capi.load()
    fields, save, _, _ = _msa_arrays(coupler)
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_msa_diagnose(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), _msa_table(fields),
                                       _msa_table(save), torch.cuda.current_stream(coupler.device).cuda_stream))


def msa_accelerate(coupler, group=None):
    """After the last module of a CRM step: the change of the level means over the step, applied once more crm_accel_factor times
    (temp, water vapour with its negative values filled from the level, and with crm_accel_uv the winds).  Returns True where the
    acceleration ceased -- a temperature tendency beyond crm_accel_max_ttend, or not a number, in ANY member -- and nothing was applied;
    the flag stays up until the next msa_init.  group: the ensemble is sharded over the ranks of this torch.distributed group; the
    flag goes through one 4-byte all-reduce(MAX) between the tendencies and the apply, like the dycore's time step
    (pam_amd/parallel.py).  One 4-byte read-back synchronises the stream."""
    import torch.distributed as dist
    lib = capi.load()
    fields, save, tend, cease = _msa_arrays(coupler)
    nens, nx, ny, nz = coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz()
    mine = C.c_int(0)
    with torch.cuda.device(coupler.device):
        stream = torch.cuda.current_stream(coupler.device).cuda_stream
        check(lib.pam_amd_msa_tendencies(nens, nx, ny, nz, _msa_table(fields), _msa_table(save), _msa_table(tend),
                                         float(coupler.get_option("crm_accel_max_ttend")), cease.data_ptr(), C.byref(mine), stream))
        flag = mine.value
        if group is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            t = cease if dist.get_backend(group) == "nccl" else torch.tensor([flag], dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            flag = int(t.item())
            if flag and not mine.value:
                cease.fill_(1)
        if flag:
            coupler.set_option("crm_accel_ceaseflag", True)
            return True
        check(lib.pam_amd_msa_apply(nens, nx, ny, nz, _msa_table(fields), _msa_table(tend), float(coupler.get_option("crm_accel_factor")),
                                    1 if coupler.get_option("crm_accel_uv") else 0, cease.data_ptr(), stream))
    return False


# ---- CRM variance transport (Hannah and Pressel 2022; E3SM-MMF's use_MMF_VT, bulk form).  Not part of the reference tree: the contract
# is this project's (include/pam_amd_modules.h; numpy restatement: tests/vt_ref.py)
VT_QUANTITIES = ("t", "q", "u")
VT_ENTRIES = (("mean", "level mean"), ("var", "level variance"), ("var_start", "level variance at the start of the GCM step"),
              ("scale", "factor of the anomalies in the last CRM step"), ("tend", "variance tendency from the GCM"),
              ("feedback", "variance tendency of the CRM over the GCM step"))


def _vt_arrays(coupler):
    """-> fields[5], {entry: [t, q, u or None]}, use_u"""
    from .coupler import endrun
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("vt_var_start_t"):
        endrun("ERROR: variance transport: call vt_init first")
    use_u = bool(coupler.get_option("crm_vt_u"))
    micro = coupler.get_option("micro") if coupler.option_exists("micro") else "none"
    if micro not in MSA_CONDENSATE:
        endrun("ERROR: variance transport only knows the kessler, p3 and none microphysics")
    cloud, ice = MSA_CONDENSATE[micro]
    fields = [dm.get("temp"), dm.get("water_vapor"), dm.get(cloud, readonly=True) if cloud else None,
              dm.get(ice, readonly=True) if ice else None, dm.get("uvel") if use_u else None]
    tables = {n: [dm.get("vt_%s_%s" % (n, q)) if (q != "u" or use_u) else None for q in VT_QUANTITIES] for n, _ in VT_ENTRIES}
    return fields, tables, use_u


def vt_init(coupler):
    """First in every GCM step: registers "vt_mean_x", "vt_var_x", "vt_var_start_x", "vt_scale_x", "vt_tend_x" (the GCM's input, zero-filled
    when registered) and "vt_feedback_x" (nz,nens), x = t, q and (with crm_vt_u) u, on first use, and fills "vt_var_start_x" with the
    variances the CRM starts from.  Options: "crm_vt_u" (default False), "crm_vt_scale_limit" (in (0,1), default 0.05)."""
    from .coupler import endrun
    if not coupler.option_exists("crm_vt_u"):
        coupler.set_option("crm_vt_u", False)
    if not coupler.option_exists("crm_vt_scale_limit"):
        coupler.set_option("crm_vt_scale_limit", 0.05)
    lim = float(coupler.get_option("crm_vt_scale_limit"))
    if not 0 < lim < 1:
        endrun("ERROR: variance transport: crm_vt_scale_limit must lie in (0, 1)")
    nz, nens = coupler.get_nz(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("vt_var_start_t"):
        for q in VT_QUANTITIES[:3 if coupler.get_option("crm_vt_u") else 2]:
            for n, desc in VT_ENTRIES:
                dm.register_and_allocate("vt_%s_%s" % (n, q), desc, (nz, nens), ("z", "nens"))
            dm.get("vt_tend_" + q).zero_()
    lib = capi.load()
    fields, tb, use_u = _vt_arrays(coupler)
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_vt_diagnose(nens, coupler.get_nx(), coupler.get_ny(), nz, _msa_table(fields), int(use_u), _msa_table(tb["mean"]),
                                      _msa_table(tb["var_start"]), torch.cuda.current_stream(coupler.device).cuda_stream))


def vt_apply_forcing(coupler, dt=None):
    """Last in a CRM step: the level statistics, the scale sqrt(1 + dt tend / var) clamped to 1 +- crm_vt_scale_limit, and the anomalies of
    temp, total water (through the vapour, its negative values filled from the level) and, with crm_vt_u, uvel stretched by it.
    dt: the model time the step counts (default: option "crm_dt"; an accelerated step passes its weight times crm_dt)."""
    lib = capi.load()
    fields, tb, use_u = _vt_arrays(coupler)
    nens, nx, ny, nz = coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz()
    dt = float(coupler.get_option("crm_dt") if dt is None else dt)
    with torch.cuda.device(coupler.device):
        stream = torch.cuda.current_stream(coupler.device).cuda_stream
        check(lib.pam_amd_vt_forcing(nens, nx, ny, nz, _msa_table(fields), int(use_u), _msa_table(tb["tend"]), dt,
                                     float(coupler.get_option("crm_vt_scale_limit")), _msa_table(tb["mean"]), _msa_table(tb["var"]),
                                     _msa_table(tb["scale"]), stream))
        check(lib.pam_amd_vt_apply(nens, nx, ny, nz, _msa_table(fields), int(use_u), _msa_table(tb["mean"]), _msa_table(tb["scale"]), stream))


def vt_compute_feedback(coupler):
    """At the end of a GCM step: "vt_feedback_x" = ("vt_var_x" - "vt_var_start_x") / gcm_physics_dt, with "vt_var_x" taken now."""
    lib = capi.load()
    fields, tb, use_u = _vt_arrays(coupler)
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_vt_feedback(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), _msa_table(fields), int(use_u),
                                      _msa_table(tb["var_start"]), float(coupler.get_option("gcm_physics_dt")), _msa_table(tb["mean"]),
                                      _msa_table(tb["var"]), _msa_table(tb["feedback"]),
                                      torch.cuda.current_stream(coupler.device).cuda_stream))


# ---- horizontal hyperdiffusion (the fourth-difference damping of the 2 dx mode E3SM-MMF's CRM applies between the sponge layer and the
# physics).  Not part of the reference tree: the contract is this project's (include/pam_amd_modules.h; numpy
# restatement: tests/hd_ref.py)
HYPERDIFFUSION_FIELDS = ("temp", "uvel", "vvel", "wvel")


def hyperdiffusion_init(coupler, tau):
    """Once: sets the option "crm_hyperdiff_timescale" (seconds; the 2 dx mode of one direction decays by dt / tau per call)."""
    from .coupler import endrun
    if not float(tau) > 0:
        endrun("ERROR: hyperdiffusion: crm_hyperdiff_timescale must be positive")
    coupler.set_option("crm_hyperdiff_timescale", float(tau))


def hyperdiffusion(coupler, dt=None):
    """Once per CRM step, after the sponge layer and the surface friction and before SGS and microphysics: temp, uvel, vvel, wvel and every
    registered tracer, in place; a tracer registered as positive is handed on non-negative.  density_dry is never touched.
    dt: default the option "crm_dt"."""
    from .coupler import endrun
    if not coupler.option_exists("crm_hyperdiff_timescale"):
        endrun("ERROR: hyperdiffusion: call hyperdiffusion_init first")
    lib = capi.load()
    dm = coupler.get_data_manager_device_readwrite()
    tracers = coupler.get_tracer_names()
    tens = [dm.get(n) for n in HYPERDIFFUSION_FIELDS] + [dm.get(n) for n in tracers]
    positive = [0] * len(HYPERDIFFUSION_FIELDS) + [1 if coupler.get_tracer_info(n)[2] else 0 for n in tracers]
    dt = float(coupler.get_option("crm_dt") if dt is None else dt)
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_hyperdiffusion(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), len(tens), _ptr_table(tens),
                                         (C.c_ubyte * len(tens))(*positive), dt, float(coupler.get_option("crm_hyperdiff_timescale")),
                                         torch.cuda.current_stream(coupler.device).cuda_stream))


# ---- the CRM-to-GCM handoff: the radiation inputs on the rad column groups (E3SM-MMF's crm_rad_* arrays) and the CRM feedback tendencies.
# Not part of the reference tree: the contract is this project's (include/pam_amd_modules.h; numpy restatement:
# tests/rad_ref.py)
RAD_AGGREGATES = ("rad_temperature", "rad_qv", "rad_qc", "rad_qi", "rad_cld")
CRM_FEEDBACK_QUANTITIES = ("t", "qv", "qc", "qi", "u", "v")
CRM_FEEDBACK_GCM = ("gcm_temp", "gcm_density_dry", "gcm_water_vapor", "gcm_cloud_water", "gcm_cloud_ice", "gcm_uvel", "gcm_vvel")


def _handoff_condensate(coupler, who):
    from .coupler import endrun
    micro = coupler.get_option("micro") if coupler.option_exists("micro") else "none"
    if micro not in MSA_CONDENSATE:
        endrun("ERROR: %s only knows the kessler, p3 and none microphysics" % who)
    return MSA_CONDENSATE[micro]


def _rad_aggregate_names(coupler):
    """-> the sizes of the forced radiation plug-in, (cloud, ice) and the names of the aggregates this microphysics has"""
    from .coupler import endrun
    from .physics import _forced_sizes
    if not (coupler.option_exists("rad_nx") and coupler.option_exists("rad_ny")):
        endrun("ERROR: rad_aggregate: options rad_nx and rad_ny are not set")
    sizes = _forced_sizes(coupler)
    cloud, ice = _handoff_condensate(coupler, "rad_aggregate")
    names = [n for n in RAD_AGGREGATES if not (n == "rad_qc" and cloud is None) and not (n == "rad_qi" and ice is None)]
    return sizes, cloud, ice, names


def rad_aggregate_init(coupler):
    """First in every GCM step: registers "rad_temperature", "rad_qv", "rad_qc", "rad_qi" and "rad_cld" (nz,rad_ny,rad_nx,nens) on first
    use -- "rad_qc" / "rad_qi" only where the microphysics (option "micro") has the species -- and zeroes them.  Options "rad_nx",
    "rad_ny": >= 1 and divisors of the CRM grid, as the forced Radiation plug-in reads them."""
    from .coupler import endrun
    (nens, nz, ny, nx, rad_ny, rad_nx), _, _, names = _rad_aggregate_names(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    shape = [nz, rad_ny, rad_nx, nens]
    for n in names:
        if dm.entry_exists(n) and dm.get_shape(n) != shape:
            endrun("ERROR: rad_aggregate: %s exists with a shape other than (nz,rad_ny,rad_nx,nens)" % n)
    for n in names:
        if not dm.entry_exists(n):
            dm.register_and_allocate(n, "radiation input on the rad column groups, averaged over the GCM step", tuple(shape),
                                     ("z", "rad_y", "rad_x", "nens"))
    rad = [dm.get(n) for n in names]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_time_average_zero(len(rad), _sizes([shape] * len(rad)), _ptr_table(rad),
                                                    torch.cuda.current_stream(coupler.device).cuda_stream))


def rad_aggregate(coupler, weight=1):
    """After the last module of every CRM step: rad_x += A(x) * (crm_dt / gcm_physics_dt * weight) with A the mean over the rad column
    group of temp, rho_v / (rho_d + rho_v), rho_c / (..), rho_i / (..) and the cloud fraction -- the entry "cldfrac" where the
    DataManager has it, otherwise 1 where a cell's condensate is positive and 0 where it is not.  The factor is
    time_average_accumulate's, so weight takes MsaClock's step weight.  Every misuse raises before the launch."""
    import math
    from .coupler import endrun
    (nens, nz, ny, nx, rad_ny, rad_nx), cloud, ice, names = _rad_aggregate_names(coupler)
    crm_dt = float(coupler.get_option("crm_dt"))
    gcm_dt = float(coupler.get_option("gcm_physics_dt"))
    if not gcm_dt > 0:
        endrun("ERROR: rad_aggregate: gcm_physics_dt must be positive")
    factor = crm_dt / gcm_dt * float(weight)
    if not math.isfinite(factor):
        endrun("ERROR: rad_aggregate: crm_dt / gcm_physics_dt x weight is not finite")
    dm = coupler.get_data_manager_device_readwrite()
    for n in names:
        if not dm.entry_exists(n):
            endrun("ERROR: %s does not exist: call rad_aggregate_init first" % n)
        if dm.get_shape(n) != [nz, rad_ny, rad_nx, nens]:
            endrun("ERROR: rad_aggregate: %s is %s, not (nz,rad_ny,rad_nx,nens) = %s" % (n, dm.get_shape(n), [nz, rad_ny, rad_nx, nens]))
    has_cldfrac = dm.entry_exists("cldfrac")
    if has_cldfrac and dm.get_shape("cldfrac") != [nz, ny, nx, nens]:
        endrun("ERROR: rad_aggregate: cldfrac is %s, not (nz,ny,nx,nens)" % dm.get_shape("cldfrac"))
    fields = [dm.get("temp", readonly=True), dm.get("density_dry", readonly=True), dm.get("water_vapor", readonly=True),
              dm.get(cloud, readonly=True) if cloud else None, dm.get(ice, readonly=True) if ice else None,
              dm.get("cldfrac", readonly=True) if has_cldfrac else None]
    rad = [dm.get(n) if n in names else None for n in RAD_AGGREGATES]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_radiation_aggregate(nens, nx, ny, nz, rad_nx, rad_ny, _msa_table(fields), _msa_table(rad), factor,
                                                      torch.cuda.current_stream(coupler.device).cuda_stream))


def _crm_feedback_quantities(coupler):
    cloud, ice = _handoff_condensate(coupler, "crm_feedback")
    return cloud, ice, [q for q in CRM_FEEDBACK_QUANTITIES if not (q == "qc" and cloud is None) and not (q == "qi" and ice is None)]


def crm_feedback_init(coupler):
    """Registers "crm_feedback_mean_{t,qv,qc,qi,u,v}" and "crm_feedback_tend_{t,qv,qc,qi,u,v}" (nz,nens) on first use; qc and qi only
    where the microphysics (option "micro") has the species."""
    from .coupler import endrun
    nz, nens = coupler.get_nz(), coupler.get_nens()
    if min(nz, nens) < 1:
        endrun("ERROR: crm_feedback: the coupler state is not allocated")
    _, _, quantities = _crm_feedback_quantities(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    names = ["crm_feedback_%s_%s" % (what, q) for q in quantities for what in ("mean", "tend")]
    for n in names:
        if dm.entry_exists(n) and dm.get_shape(n) != [nz, nens]:
            endrun("ERROR: crm_feedback: %s exists with a shape other than (nz,nens)" % n)
    for n in names:
        if not dm.entry_exists(n):
            dm.register_and_allocate(n, "CRM level mean, and its distance from the GCM's value over the GCM step", (nz, nens), ("z", "nens"))


def compute_crm_feedback(coupler):
    """At the end of a GCM step: "crm_feedback_mean_x" = the level mean of temp, rho_v / (rho_d + rho_v), rho_c / (..), rho_i / (..), uvel,
    vvel; "crm_feedback_tend_x" = (mean_x - the GCM's value from the "gcm_*" entries) / gcm_physics_dt: the converse of
    compute_gcm_forcing_tendencies.  One read of the fields, one launch."""
    import math
    from .coupler import endrun
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("crm_feedback_tend_t"):
        endrun("ERROR: crm_feedback: call crm_feedback_init first")
    cloud, ice, quantities = _crm_feedback_quantities(coupler)
    gcm_dt = float(coupler.get_option("gcm_physics_dt"))
    if not (gcm_dt > 0 and math.isfinite(gcm_dt)):
        endrun("ERROR: crm_feedback: gcm_physics_dt must be finite and positive")
    nz, nens = coupler.get_nz(), coupler.get_nens()
    for q in quantities:
        for what in ("mean", "tend"):
            n = "crm_feedback_%s_%s" % (what, q)
            if not dm.entry_exists(n):
                endrun("ERROR: crm_feedback: %s does not exist: the microphysics changed since crm_feedback_init" % n)
            if dm.get_shape(n) != [nz, nens]:
                endrun("ERROR: crm_feedback: %s is %s, not (nz,nens)" % (n, dm.get_shape(n)))
    fields = [dm.get("temp", readonly=True), dm.get("density_dry", readonly=True), dm.get("water_vapor", readonly=True),
              dm.get(cloud, readonly=True) if cloud else None, dm.get(ice, readonly=True) if ice else None,
              dm.get("uvel", readonly=True), dm.get("vvel", readonly=True)]
    gcm = [None if (n == "gcm_cloud_water" and cloud is None) or (n == "gcm_cloud_ice" and ice is None) else dm.get(n, readonly=True)
           for n in CRM_FEEDBACK_GCM]
    mean = [dm.get("crm_feedback_mean_" + q) if q in quantities else None for q in CRM_FEEDBACK_QUANTITIES]
    tend = [dm.get("crm_feedback_tend_" + q) if q in quantities else None for q in CRM_FEEDBACK_QUANTITIES]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_crm_feedback(nens, coupler.get_nx(), coupler.get_ny(), nz, _msa_table(fields), _msa_table(gcm), gcm_dt,
                                               _msa_table(mean), _msa_table(tend), torch.cuda.current_stream(coupler.device).cuda_stream))


# ---- the CRM column diagnostics: cloud cover, water paths, precipitable water and surface precipitation per GCM column (the per-step
# aggregation of E3SM-MMF's pam_statistics).  Not part of the reference tree: the contract is this project's (include/pam_amd_modules.h,
# DESIGN.md section 8; numpy restatement: tests/coldiag_ref.py)
COLUMN_DIAGNOSTICS = ("diag_cldtot", "diag_cldlow", "diag_cldmed", "diag_cldhgh", "diag_lwp", "diag_iwp", "diag_pw", "diag_precip_liq",
                      "diag_precip_ice")
COLUMN_DIAGNOSTICS_DEFAULTS = (("crm_diag_p_low", 70000.0), ("crm_diag_p_high", 40000.0), ("crm_diag_cwp_threshold", 1.0e-3))


def _column_diagnostics_names(coupler):
    """-> (nens, nz, ny, nx), (cloud, ice), the two precipitation entries (None where the DataManager has none) and the nine outputs'
    names in the order of the C ABI, None where the coupler lacks the inputs"""
    from .coupler import endrun
    nens, nz, ny, nx = coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx()
    if min(nens, nz, ny, nx) < 1:
        endrun("ERROR: column_diagnostics: the coupler state is not allocated")
    cloud, ice = _handoff_condensate(coupler, "column_diagnostics")
    dm = coupler.get_data_manager_device_readwrite()
    liq = "precl" if dm.entry_exists("precl") else ("precip_liq_surf_out" if dm.entry_exists("precip_liq_surf_out") else None)
    pice = "preci" if dm.entry_exists("preci") else ("precip_ice_surf_out" if dm.entry_exists("precip_ice_surf_out") else None)
    for n in (liq, pice):
        if n is not None and dm.get_shape(n) != [ny, nx, nens]:
            endrun("ERROR: column_diagnostics: %s is %s, not (ny,nx,nens)" % (n, dm.get_shape(n)))
    there = [cloud is not None or ice is not None] * 4 + [cloud is not None, ice is not None, True, liq is not None, pice is not None]
    return (nens, nz, ny, nx), (cloud, ice), (liq, pice), [n if t else None for n, t in zip(COLUMN_DIAGNOSTICS, there)]


def column_diagnostics_init(coupler):
    """First in every GCM step: registers "diag_cldtot", "diag_cldlow", "diag_cldmed", "diag_cldhgh", "diag_lwp", "diag_iwp", "diag_pw",
    "diag_precip_liq" and "diag_precip_ice" (nens) on first use -- only those whose inputs the coupler has: no cloud cover without a
    condensate (option "micro"), no path without its species, no precipitation without "precl" or "precip_liq_surf_out" /
    "precip_ice_surf_out" -- and zeroes them.  Sets the options "crm_diag_p_low" = 70000, "crm_diag_p_high" = 40000 and
    "crm_diag_cwp_threshold" = 1e-3 where they are unset."""
    from .coupler import endrun
    (nens, _, _, _), _, _, names = _column_diagnostics_names(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    names = [n for n in names if n is not None]
    for n in names:
        if dm.entry_exists(n) and dm.get_shape(n) != [nens]:
            endrun("ERROR: column_diagnostics: %s exists with a shape other than (nens)" % n)
    for opt, value in COLUMN_DIAGNOSTICS_DEFAULTS:
        if not coupler.option_exists(opt):
            coupler.set_option(opt, value)
    for n in names:
        if not dm.entry_exists(n):
            dm.register_and_allocate(n, "CRM column diagnostic, averaged over the columns and the GCM step", (nens,), ("nens",))
    out = [dm.get(n) for n in names]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_time_average_zero(len(out), _sizes([[nens]] * len(out)), _ptr_table(out),
                                                    torch.cuda.current_stream(coupler.device).cuda_stream))


def column_diagnostics(coupler, weight=1):
    """After the last module of every CRM step: diag_x += M(x) * (crm_dt / gcm_physics_dt * weight) with M the mean over the CRM columns
    of the column's cloud covers (the greatest cloud fraction of the levels of a pressure class where the class's condensed water path
    exceeds crm_diag_cwp_threshold), water paths and surface precipitation.  The factor is time_average_accumulate's, so weight takes
    MsaClock's step weight.  Every misuse raises before the launch."""
    import math
    from .coupler import endrun
    (nens, nz, ny, nx), (cloud, ice), (liq, pice), names = _column_diagnostics_names(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("diag_pw"):
        endrun("ERROR: diag_pw does not exist: call column_diagnostics_init first")
    for opt in ("R_d", "R_v") + tuple(o for o, _ in COLUMN_DIAGNOSTICS_DEFAULTS):
        if not coupler.option_exists(opt):
            endrun("ERROR: column_diagnostics: option %s is not set" % opt)
    R_d, R_v = float(coupler.get_option("R_d")), float(coupler.get_option("R_v"))
    p_low, p_high = float(coupler.get_option("crm_diag_p_low")), float(coupler.get_option("crm_diag_p_high"))
    threshold = float(coupler.get_option("crm_diag_cwp_threshold"))
    if not all(math.isfinite(v) for v in (R_d, R_v, p_low, p_high)):
        endrun("ERROR: column_diagnostics: R_d, R_v, crm_diag_p_low and crm_diag_p_high must be finite")
    if p_high > p_low:
        endrun("ERROR: column_diagnostics: crm_diag_p_high must not exceed crm_diag_p_low")
    if not threshold >= 0:
        endrun("ERROR: column_diagnostics: crm_diag_cwp_threshold must be >= 0")
    crm_dt = float(coupler.get_option("crm_dt"))
    gcm_dt = float(coupler.get_option("gcm_physics_dt"))
    if not gcm_dt > 0:
        endrun("ERROR: column_diagnostics: gcm_physics_dt must be positive")
    factor = crm_dt / gcm_dt * float(weight)
    if not math.isfinite(factor):
        endrun("ERROR: column_diagnostics: crm_dt / gcm_physics_dt x weight is not finite")
    for n in names:
        if n is None:
            continue
        if not dm.entry_exists(n):
            endrun("ERROR: %s does not exist: call column_diagnostics_init first" % n)
        if dm.get_shape(n) != [nens]:
            endrun("ERROR: column_diagnostics: %s is %s, not (nens)" % (n, dm.get_shape(n)))
    has_cldfrac = dm.entry_exists("cldfrac")
    if has_cldfrac and dm.get_shape("cldfrac") != [nz, ny, nx, nens]:
        endrun("ERROR: column_diagnostics: cldfrac is %s, not (nz,ny,nx,nens)" % dm.get_shape("cldfrac"))
    fields = [dm.get("temp", readonly=True), dm.get("density_dry", readonly=True), dm.get("water_vapor", readonly=True),
              dm.get(cloud, readonly=True) if cloud else None, dm.get(ice, readonly=True) if ice else None,
              dm.get("cldfrac", readonly=True) if has_cldfrac else None]
    precip = [dm.get(n, readonly=True) if n else None for n in (liq, pice)]
    out = [dm.get(n) if n else None for n in names]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_column_diagnostics(nens, nx, ny, nz, _msa_table(fields),
                                                     dm.get("vertical_interface_height", readonly=True).data_ptr(), _msa_table(precip),
                                                     R_d, R_v, p_low, p_high, threshold, _msa_table(out), factor,
                                                     torch.cuda.current_stream(coupler.device).cuda_stream))


# ---- the CRM flux profiles: the convective mass fluxes by conditional sampling (SAM / E3SM-MMF's mcup, mcdn, mcuup, mcudn), the cloud
# fraction profile, the resolved vertical fluxes of heat, total water and horizontal momentum and the resolved turbulence kinetic energy.
# Not part of the reference tree: the contract is this project's (include/pam_amd_modules.h; numpy restatement:
# tests/fluxprof_ref.py)
FLUX_PROFILES = ("prof_mcup", "prof_mcdn", "prof_mcuup", "prof_mcudn", "prof_cld", "prof_flux_t", "prof_flux_qt", "prof_flux_u", "prof_flux_v",
                 "prof_tke")
FLUX_PROFILES_DEFAULTS = (("crm_prof_qc_threshold", 1.0e-5),)


def _flux_profiles_names(coupler):
    """-> (nens, nz, ny, nx), (cloud, ice) and the ten outputs' names in the order of the C ABI, None where the microphysics lacks the
    inputs (no condensate: no prof_mcup, prof_mcdn, prof_cld)"""
    from .coupler import endrun
    nens, nz, ny, nx = coupler.get_nens(), coupler.get_nz(), coupler.get_ny(), coupler.get_nx()
    if min(nens, nz, ny, nx) < 1:
        endrun("ERROR: flux_profiles: the coupler state is not allocated")
    cloud, ice = _handoff_condensate(coupler, "flux_profiles")
    cloudy = cloud is not None or ice is not None
    return (nens, nz, ny, nx), (cloud, ice), [n if (cloudy or n not in ("prof_mcup", "prof_mcdn", "prof_cld")) else None for n in FLUX_PROFILES]


def flux_profiles_init(coupler):
    """First in every GCM step: registers "prof_mcup", "prof_mcdn", "prof_mcuup", "prof_mcudn", "prof_cld", "prof_flux_t", "prof_flux_qt",
    "prof_flux_u", "prof_flux_v" and "prof_tke" (nz,nens) on first use -- only those whose inputs the microphysics (option "micro") has:
    no prof_mcup, prof_mcdn and prof_cld without a condensate -- and zeroes them.  Sets the option "crm_prof_qc_threshold" = 1e-5 where it
    is unset."""
    from .coupler import endrun
    (nens, nz, _, _), _, names = _flux_profiles_names(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    names = [n for n in names if n is not None]
    for n in names:
        if dm.entry_exists(n) and dm.get_shape(n) != [nz, nens]:
            endrun("ERROR: flux_profiles: %s exists with a shape other than (nz,nens)" % n)
    for opt, value in FLUX_PROFILES_DEFAULTS:
        if not coupler.option_exists(opt):
            coupler.set_option(opt, value)
    for n in names:
        if not dm.entry_exists(n):
            dm.register_and_allocate(n, "CRM flux profile, averaged over the columns and the GCM step", (nz, nens), ("z", "nens"))
    out = [dm.get(n) for n in names]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_time_average_zero(len(out), _sizes([[nz, nens]] * len(out)), _ptr_table(out),
                                                    torch.cuda.current_stream(coupler.device).cuda_stream))


def flux_profiles(coupler, weight=1):
    """After the last module of every CRM step: prof_x += value * (crm_dt / gcm_physics_dt * weight) with, per level and member, the mass
    flux rho w averaged over the CRM columns of each class (cloudy where the condensate exceeds crm_prof_qc_threshold x rho, up where
    w > 0), the cloudy fraction, the resolved fluxes of temp, total water, uvel and vvel and the resolved turbulence kinetic energy.  The
    factor is time_average_accumulate's, so weight takes MsaClock's step weight.  Every misuse raises before the launch."""
    import math
    from .coupler import endrun
    (nens, nz, ny, nx), (cloud, ice), names = _flux_profiles_names(coupler)
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("prof_tke"):
        endrun("ERROR: prof_tke does not exist: call flux_profiles_init first")
    for opt, _ in FLUX_PROFILES_DEFAULTS:
        if not coupler.option_exists(opt):
            endrun("ERROR: flux_profiles: option %s is not set" % opt)
    threshold = float(coupler.get_option("crm_prof_qc_threshold"))
    if not (threshold >= 0 and math.isfinite(threshold)):
        endrun("ERROR: flux_profiles: crm_prof_qc_threshold must be finite and >= 0")
    crm_dt = float(coupler.get_option("crm_dt"))
    gcm_dt = float(coupler.get_option("gcm_physics_dt"))
    if not gcm_dt > 0:
        endrun("ERROR: flux_profiles: gcm_physics_dt must be positive")
    factor = crm_dt / gcm_dt * float(weight)
    if not math.isfinite(factor):
        endrun("ERROR: flux_profiles: crm_dt / gcm_physics_dt x weight is not finite")
    for n in FLUX_PROFILES:
        if n not in names and dm.entry_exists(n):
            endrun("ERROR: flux_profiles: %s exists, but this microphysics has no condensate: it changed since flux_profiles_init" % n)
    for n in names:
        if n is None:
            continue
        if not dm.entry_exists(n):
            endrun("ERROR: %s does not exist: call flux_profiles_init first" % n)
        if dm.get_shape(n) != [nz, nens]:
            endrun("ERROR: flux_profiles: %s is %s, not (nz,nens)" % (n, dm.get_shape(n)))
    fields = [dm.get("density_dry", readonly=True), dm.get("water_vapor", readonly=True),
              dm.get(cloud, readonly=True) if cloud else None, dm.get(ice, readonly=True) if ice else None,
              dm.get("temp", readonly=True), dm.get("uvel", readonly=True), dm.get("vvel", readonly=True), dm.get("wvel", readonly=True)]
    out = [dm.get(n) if n else None for n in names]
    with torch.cuda.device(coupler.device):
        check(capi.load().pam_amd_flux_profiles(nens, nx, ny, nz, _msa_table(fields), threshold, _msa_table(out), factor,
                                                torch.cuda.current_stream(coupler.device).cuda_stream))


# ---- bulk surface fluxes over a slab ocean: the surface that SGSSmagorinsky(surface_fluxes=True) and RadiationGray name.  Not part of
# the reference tree: the contract is this project's (include/pam_amd_modules.h at pam_amd_surface_fluxes; numpy
# restatement: tests/surface_ref.py)
SURFACE_FLUX_FIELDS = (("sfc_shf", "input surface sensible heat flux [W/m2]"), ("sfc_lhf", "input surface latent heat flux [W/m2]"))
SURFACE_RADIATION = ("rad_lw_down_sfc", "rad_lw_up_sfc", "rad_sw_down_sfc", "rad_sw_up_sfc")
SURFACE_Z0 = 1.0e-4                               # where neither the entry "z0" nor the argument gives one [m]
SURFACE_RHO_W, SURFACE_C_W = 1000.0, 4186.0       # slab_heat_capacity = rho_w c_w depth
SURFACE_LATVAP = 2501000.0                        # where the option "latvap" is absent, as SGSSmagorinsky has it


def surface_transfer_parameters(zmid0, z0):
    """host arithmetic, once: lnz = log(zmid0 / z0); cn = (0.4 / lnz)^2; cstar = ((5.3 * 9.4) cn) sqrt(zmid0 / z0); numpy arrays (nens)"""
    import numpy as np
    r = np.asarray(zmid0, dtype=np.float64) / np.asarray(z0, dtype=np.float64)
    k = 0.4 / np.log(r)
    cn = k * k
    return cn, ((5.3 * 9.4) * cn) * np.sqrt(r)


def surface_fluxes_init(coupler, sst=300.0, z0=None, slab_depth=0.0, gust=1.0, wetness=0.98):
    """Once, after the grid is set: registers "sfc_temp" (ny,nx,nens) where absent and fills it with sst (a float or nens values; an
    existing entry keeps its values), "sfc_shf" and "sfc_lhf" where absent under the names and descriptions SGSSmagorinsky uses, and
    "sfc_cn" and "sfc_cstar" (nens), the transfer parameters of every member, formed on the host from row 0 of
    "vertical_midpoint_height" and the roughness height: the entry "z0" where surface_friction_init has made one, else the argument z0 (a
    float or nens values), else 1e-4 m.  Options "sfc_slab_depth" [m], "sfc_gust" [m/s] and "sfc_wetness" are set only where absent."""
    import numpy as np
    from .coupler import endrun
    ny, nx, nens = coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("sfc_temp"):
        dm.register_and_allocate("sfc_temp", "surface temperature [K]", (ny, nx, nens), ("y", "x", "nens"))
        t = torch.as_tensor(sst, dtype=torch.float64, device=coupler.device)
        if t.dim() > 1 or (t.dim() == 1 and t.numel() != nens):
            endrun("ERROR: surface_fluxes_init: sst needs one value or nens values")
        dm.get("sfc_temp").copy_(t.expand(ny, nx, nens))
    for name, desc in SURFACE_FLUX_FIELDS:
        if not dm.entry_exists(name):
            dm.register_and_allocate(name, desc, (ny, nx, nens), ("y", "x", "nens"))
    if dm.entry_exists("z0"):
        z0 = dm.get("z0", readonly=True).cpu().numpy()
    else:
        z0 = np.broadcast_to(np.asarray(SURFACE_Z0 if z0 is None else z0, dtype=np.float64), (nens,))
    if z0.shape != (nens,) or not (z0 > 0).all():
        endrun("ERROR: surface_fluxes_init: z0 needs one positive value or nens positive values")
    zmid0 = dm.get("vertical_midpoint_height", readonly=True)[0].cpu().numpy()
    if not (zmid0 > z0).all():
        endrun("ERROR: surface_fluxes_init: the lowest level must lie above the roughness height")
    for name, desc, a in zip(("sfc_cn", "sfc_cstar"), ("neutral surface transfer coefficient [1]", "unstable-branch coefficient of the surface transfer [1]"),
                             surface_transfer_parameters(zmid0, z0)):
        if not dm.entry_exists(name):
            dm.register_and_allocate(name, desc, (nens,), ("nens",))
        dm.get(name).copy_(torch.as_tensor(a, dtype=torch.float64))
    for name, value in (("sfc_slab_depth", float(slab_depth)), ("sfc_gust", float(gust)), ("sfc_wetness", float(wetness))):
        if not coupler.option_exists(name):
            coupler.set_option(name, value)


def surface_fluxes(coupler, dt=None):
    """Once per CRM step, before the surface friction and the SGS: "sfc_shf" and "sfc_lhf" from the lowest level and "sfc_temp", and, where
    option "sfc_slab_depth" > 0, "sfc_temp" stepped by the net energy with slab_heat_capacity = 1000.0 * 4186.0 * slab_depth.  The entries
    "rad_lw_down_sfc"/"rad_lw_up_sfc" and "rad_sw_down_sfc"/"rad_sw_up_sfc" are handed over by pairs where they exist.  Options "grav",
    "cp_d", "R_v", and "latvap" where it exists.  dt: default the option "crm_dt"."""
    from .coupler import endrun
    dm = coupler.get_data_manager_device_readwrite()
    if not dm.entry_exists("sfc_cn"):
        endrun("ERROR: surface_fluxes: call surface_fluxes_init first")
    lib = capi.load()
    inputs = [dm.get(n, readonly=True) for n in ("temp", "density_dry", "water_vapor", "uvel", "vvel", "vertical_midpoint_height", "sfc_cn",
                                                 "sfc_cstar")]
    rad = []
    for down, up in (SURFACE_RADIATION[:2], SURFACE_RADIATION[2:]):
        both = dm.entry_exists(down) and dm.entry_exists(up)
        rad += [dm.get(down, readonly=True).data_ptr(), dm.get(up, readonly=True).data_ptr()] if both else [None, None]
    dt = float(coupler.get_option("crm_dt") if dt is None else dt)
    latvap = float(coupler.get_option("latvap")) if coupler.option_exists("latvap") else SURFACE_LATVAP
    cap = SURFACE_RHO_W * SURFACE_C_W * float(coupler.get_option("sfc_slab_depth"))
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_surface_fluxes(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(),
                                         *[a.data_ptr() for a in inputs], dm.get("sfc_temp").data_ptr(), *rad,
                                         float(coupler.get_option("sfc_gust")), float(coupler.get_option("sfc_wetness")),
                                         float(coupler.get_option("grav")), float(coupler.get_option("cp_d")), float(coupler.get_option("R_v")),
                                         latvap, cap, dt, dm.get("sfc_shf").data_ptr(), dm.get("sfc_lhf").data_ptr(),
                                         torch.cuda.current_stream(coupler.device).cuda_stream))


# ---- large-scale forcing: subsidence, horizontally uniform tendencies, nudging of the level means and the Coriolis force about a
# geostrophic wind (SAM's forcing + subsidence + nudging + coriolis).  Not part of the reference tree: the contract is this project's
# (include/pam_amd_modules.h at pam_amd_ls_forcing; numpy restatement: tests/lsforcing_ref.py)
LS_PROFILES = (("ls_wsub", "large-scale vertical velocity [m/s]"), ("ls_temp_tend", "large-scale temperature tendency [K/s]"),
               ("ls_qv_tend", "large-scale tendency of the vapour mixing ratio rho_v / rho [1/s]"),
               ("ls_ug", "geostrophic wind, x [m/s]"), ("ls_vg", "geostrophic wind, y [m/s]"),
               ("ls_nudge_temp", "nudging target of the level-mean temperature [K]"),
               ("ls_nudge_qv", "nudging target of the level-mean rho_v / rho [1]"),
               ("ls_nudge_u", "nudging target of the level-mean uvel [m/s]"), ("ls_nudge_v", "nudging target of the level-mean vvel [m/s]"),
               ("ls_nudge_rate_temp", "nudging rate of temp [1/s]"), ("ls_nudge_rate_qv", "nudging rate of rho_v / rho [1/s]"),
               ("ls_nudge_rate_uv", "nudging rate of uvel and vvel [1/s]"))
LS_TARGETS = ("ls_nudge_temp", "ls_nudge_qv", "ls_nudge_u", "ls_nudge_v")                      # in the order of the C ABI's tables
LS_RATES = ("ls_nudge_rate_temp", "ls_nudge_rate_qv", "ls_nudge_rate_uv", "ls_nudge_rate_uv")
LS_INCREMENTS = ("ls_inc_temp", "ls_inc_qv", "ls_inc_u", "ls_inc_v")
LS_NUDGE_FIELDS = ("temp", "density_dry", "water_vapor", "uvel", "vvel")


def ls_forcing_init(coupler, wsub=None, temp_tend=None, qv_tend=None, ug=None, vg=None, nudge_temp=None, nudge_qv=None, nudge_u=None,
                    nudge_v=None, nudge_rate_temp=None, nudge_rate_qv=None, nudge_rate_uv=None, fcor=None):
    """Once, after the grid is set: registers the profiles that are given as DEVICE entries (nz,nens) under the names of LS_PROFILES
    ("ls_wsub", ..., the argument's name behind "ls_"), each from nz values (every member alike) or (nz,nens) values, "ls_fcor" (nens)
    from one value or nens values, and "ls_inc_*" (nz,nens) for every target.  A profile that is not given is not registered and its
    term is absent from ls_forcing.  ug and vg come as a pair and with fcor; a target comes with its rate.  From the host copies it
    holds here it sets the options "ls_courant_rate" = max |wsub| / min (zmid(k+1) - zmid(k)) over every member [1/s] and
    "ls_nudge_rate_max" [1/s], by which ls_forcing refuses a step that is too long; a host model that overwrites an entry between
    steps with values beyond them sets the two options again."""
    import numpy as np
    from .coupler import endrun
    nz, nens = coupler.get_nz(), coupler.get_nens()
    dm = coupler.get_data_manager_device_readwrite()
    given = dict(ls_wsub=wsub, ls_temp_tend=temp_tend, ls_qv_tend=qv_tend, ls_ug=ug, ls_vg=vg, ls_nudge_temp=nudge_temp, ls_nudge_qv=nudge_qv,
                 ls_nudge_u=nudge_u, ls_nudge_v=nudge_v, ls_nudge_rate_temp=nudge_rate_temp, ls_nudge_rate_qv=nudge_rate_qv,
                 ls_nudge_rate_uv=nudge_rate_uv)
    if (ug is None) != (vg is None) or (fcor is None) != (ug is None):
        endrun("ERROR: ls_forcing_init: ug, vg and fcor come together")
    for target, rate in zip(LS_TARGETS, LS_RATES):
        if given[target] is not None and given[rate] is None:
            endrun("ERROR: ls_forcing_init: %s needs %s" % (target, rate))
    host = {}
    for name, desc in LS_PROFILES:
        if given[name] is None:
            continue
        a = np.asarray(given[name], dtype=np.float64)
        if a.shape == (nz,):
            a = np.broadcast_to(a[:, None], (nz, nens))
        if a.shape != (nz, nens):
            endrun("ERROR: ls_forcing_init: %s needs nz values or (nz,nens) values" % name)
        host[name] = np.ascontiguousarray(a)
        if not dm.entry_exists(name):
            dm.register_and_allocate(name, desc, (nz, nens), ("z", "nens"))
        dm.get(name).copy_(torch.from_numpy(host[name]))
    if fcor is not None:
        f = np.broadcast_to(np.asarray(fcor, dtype=np.float64), (nens,)) if np.ndim(fcor) == 0 else np.asarray(fcor, dtype=np.float64)
        if f.shape != (nens,):
            endrun("ERROR: ls_forcing_init: fcor needs one value or nens values")
        if not dm.entry_exists("ls_fcor"):
            dm.register_and_allocate("ls_fcor", "Coriolis parameter [1/s]", (nens,), ("nens",))
        dm.get("ls_fcor").copy_(torch.from_numpy(np.ascontiguousarray(f)))
    for target, inc in zip(LS_TARGETS, LS_INCREMENTS):
        if target in host and not dm.entry_exists(inc):
            dm.register_and_allocate(inc, "nudging increment of the level mean", (nz, nens), ("z", "nens"))
    courant = 0.0
    if "ls_wsub" in host and nz > 1:
        zmid = dm.get("vertical_midpoint_height", readonly=True).cpu().numpy()
        courant = float((np.abs(host["ls_wsub"]).max(axis=0) / (zmid[1:] - zmid[:-1]).min(axis=0)).max())
    coupler.set_option("ls_courant_rate", courant)
    coupler.set_option("ls_nudge_rate_max", max([float(host[r].max()) for r in set(LS_RATES) if r in host], default=0.0))


def ls_forcing(coupler, dt=None):
    """Once per CRM step, after the sponge layer and before surface_fluxes: one call of pam_amd_ls_nudging where a target is registered,
    then one of pam_amd_ls_forcing, in place on uvel, vvel, temp and every registered tracer (the vapour is "water_vapor"; a tracer
    registered as positive is handed on non-negative).  density_dry and wvel are never written.  Refuses, before anything is launched,
    dt "ls_courant_rate" > 1 (the subsidence would overshoot) and dt "ls_nudge_rate_max" > 1.  Options "grav", "cp_d"; dt: default the
    option "crm_dt"."""
    from .coupler import endrun
    if not coupler.option_exists("ls_courant_rate"):
        endrun("ERROR: ls_forcing: call ls_forcing_init first")
    dt = float(coupler.get_option("crm_dt") if dt is None else dt)
    if not dt * float(coupler.get_option("ls_courant_rate")) <= 1.0:
        endrun("ERROR: ls_forcing: max |ls_wsub| dt exceeds the thinnest layer (dt x ls_courant_rate > 1)")
    if not dt * float(coupler.get_option("ls_nudge_rate_max")) <= 1.0:
        endrun("ERROR: ls_forcing: dt x nudging rate exceeds 1 (dt x ls_nudge_rate_max > 1)")
    lib = capi.load()
    dm = coupler.get_data_manager_device_readwrite()
    P = lambda name: dm.get(name, readonly=True).data_ptr() if dm.entry_exists(name) else None
    nens, nx, ny, nz = coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz()
    names = coupler.get_tracer_names()
    tracers = [dm.get(n) for n in names]
    positive = [1 if coupler.get_tracer_info(n)[2] else 0 for n in names]
    nudged = [dm.entry_exists(t) for t in LS_TARGETS]
    with torch.cuda.device(coupler.device):
        stream = torch.cuda.current_stream(coupler.device).cuda_stream
        inc = None
        if any(nudged):
            table = lambda entries: (C.c_void_p * 4)(*[P(n) if on else None for n, on in zip(entries, nudged)])
            inc = (C.c_void_p * 4)(*[dm.get(n).data_ptr() if on else None for n, on in zip(LS_INCREMENTS, nudged)])
            check(lib.pam_amd_ls_nudging(nens, nx, ny, nz, _msa_table([dm.get(n, readonly=True) for n in LS_NUDGE_FIELDS]), table(LS_TARGETS),
                                         table(LS_RATES), dt, inc, stream))
        check(lib.pam_amd_ls_forcing(nens, nx, ny, nz, dm.get("uvel").data_ptr(), dm.get("vvel").data_ptr(), dm.get("temp").data_ptr(),
                                     len(tracers), _ptr_table(tracers) if tracers else None,
                                     (C.c_ubyte * len(tracers))(*positive) if tracers else None, P("density_dry"), P("water_vapor"),
                                     P("vertical_midpoint_height"), P("ls_wsub"), P("ls_temp_tend"), P("ls_qv_tend"), inc, P("ls_fcor"),
                                     P("ls_ug"), P("ls_vg"), dt, float(coupler.get_option("grav")), float(coupler.get_option("cp_d")), stream))


# ---- explicit scalar momentum transport for 2-D CRMs (Tulich 2015; E3SM-MMF's use_MMF_ESMT): the large-scale u and v ride as two
# passive scalars that take the linearised pressure-gradient force every CRM step.  Not part of the reference tree: the contract is this
# project's (include/pam_amd_modules.h at pam_amd_esmt_pgf; numpy restatement: tests/esmt_ref.py)
ESMT_SCALARS = ("esmt_u", "esmt_v")
ESMT_PROFILES = (("esmt_rho_mean", "level mean of the total density [kg/m3]"), ("esmt_u_mean", "level mean of esmt_u / rho [m/s]"),
                 ("esmt_v_mean", "level mean of esmt_v / rho [m/s]"), ("esmt_u_forcing", "GCM forcing of the scalar u [m/s2]"),
                 ("esmt_v_forcing", "GCM forcing of the scalar v [m/s2]"), ("esmt_u_tend", "scalar momentum feedback, u [m/s2]"),
                 ("esmt_v_tend", "scalar momentum feedback, v [m/s2]"))


def esmt_init(coupler, kmax=None):
    """Once, BEFORE Dycore.init (the dycore takes its tracer table when it is initialised): registers the tracers "esmt_u" and "esmt_v"
    (not positive, adding no mass), the profiles of ESMT_PROFILES (nz,nens) zeroed, the tables "esmt_cos" and "esmt_sin" (nx) formed
    on the host, and the workspace "esmt_workspace" (6 kmax nz nens doubles), and sets the option "esmt_kmax" (default nx // 2: every
    wavenumber).  Refuses ny != 1: a 3-D CRM transports momentum itself."""
    import numpy as np
    from .coupler import endrun
    lib = capi.load()
    nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
    if ny != 1:
        endrun("ERROR: esmt_init: explicit scalar momentum transport is for 2-D CRMs (ny == 1)")
    if nx < 2 or nz < 2:
        endrun("ERROR: esmt_init: nx and nz must be >= 2")
    kmax = nx // 2 if kmax is None else int(kmax)
    if not 0 <= kmax <= nx // 2:
        endrun("ERROR: esmt_init: kmax must be in [0, nx // 2]")
    dm = coupler.get_data_manager_device_readwrite()
    if dm.entry_exists("esmt_cos"):
        endrun("ERROR: esmt_init: called twice")
    for n, d in zip(ESMT_SCALARS, ("large-scale u carried as a scalar [kg/m3 m/s]", "large-scale v carried as a scalar [kg/m3 m/s]")):
        coupler.add_tracer(n, d, False, False)
    for n, d in ESMT_PROFILES:
        dm.register_and_allocate(n, d, (nz, nens), ("z", "nens"))
        dm.get(n).zero_()
    cos, sin = np.empty(nx), np.empty(nx)
    check(lib.pam_amd_esmt_tables(nx, cos.ctypes.data, sin.ctypes.data))
    for n, a in (("esmt_cos", cos), ("esmt_sin", sin)):
        dm.register_and_allocate(n, "table of the transform along x", (nx,), ("x",))
        dm.get(n).copy_(torch.from_numpy(a))
    words = max(int(lib.pam_amd_esmt_workspace_doubles(nens, nz, kmax)), 1)
    dm.register_and_allocate("esmt_workspace", "spectral coefficients and right-hand sides of the pressure solve", (words,))
    coupler.set_option("esmt_kmax", kmax)


def _esmt_ready(coupler, who):
    from .coupler import endrun
    if not coupler.option_exists("esmt_kmax"):
        endrun("ERROR: %s: call esmt_init first" % who)
    return coupler.get_data_manager_device_readwrite()


def esmt_set(coupler, source="gcm"):
    """Sets both scalars to rho times a profile: source "gcm" takes "gcm_uvel" / "gcm_vvel"; source "crm" takes the level means of uvel
    and vvel (pam_amd_msa_diagnose: the slot order every level mean of the project has)."""
    from .coupler import endrun
    dm = _esmt_ready(coupler, "esmt_set")
    if source not in ("gcm", "crm"):
        endrun("ERROR: esmt_set: source must be \"gcm\" or \"crm\"")
    lib = capi.load()
    nens, nx, ny, nz = coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz()
    with torch.cuda.device(coupler.device):
        stream = torch.cuda.current_stream(coupler.device).cuda_stream
        if source == "gcm":
            src = [dm.get("gcm_uvel", readonly=True), dm.get("gcm_vvel", readonly=True)]
        else:
            u, v = dm.get("uvel", readonly=True), dm.get("vvel", readonly=True)
            # the first two means of the table are not wanted: the tendencies of the feedback take them, and are written anew before use
            rest = [dm.get("esmt_u_tend"), dm.get("esmt_v_tend")]
            src = [dm.get("esmt_u_mean"), dm.get("esmt_v_mean")]
            check(lib.pam_amd_msa_diagnose(nens, nx, ny, nz, _msa_table([u, v, None, None, u, v]), _msa_table(rest + src), stream))
        check(lib.pam_amd_esmt_set(nens, nx, ny, nz, dm.get("density_dry", readonly=True).data_ptr(), dm.get("water_vapor", readonly=True).data_ptr(),
                                   src[0].data_ptr(), src[1].data_ptr(), dm.get("esmt_u").data_ptr(), dm.get("esmt_v").data_ptr(), stream))


def _esmt_diagnose(coupler, dm, tend, feedback):
    lib = capi.load()
    P = lambda n: dm.get(n, readonly=True).data_ptr()
    gcm = (P("gcm_uvel"), P("gcm_vvel")) if tend else (None, None)
    out = (dm.get(tend[0]).data_ptr(), dm.get(tend[1]).data_ptr()) if tend else (None, None)
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_esmt_diagnose(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), P("density_dry"), P("water_vapor"),
                                        P("esmt_u"), P("esmt_v"), dm.get("esmt_rho_mean").data_ptr(), dm.get("esmt_u_mean").data_ptr(),
                                        dm.get("esmt_v_mean").data_ptr(), gcm[0], gcm[1],
                                        float(coupler.get_option("gcm_physics_dt")) if tend else 1.0, 1 if feedback else 0, out[0], out[1],
                                        torch.cuda.current_stream(coupler.device).cuda_stream))


def esmt_compute_forcing(coupler):
    """Once per GCM step: "esmt_x_forcing" = (gcm_x - M(esmt_x / rho)) / gcm_physics_dt, what the GCM applies to the scalars."""
    _esmt_diagnose(coupler, _esmt_ready(coupler, "esmt_compute_forcing"), ("esmt_u_forcing", "esmt_v_forcing"), False)


def esmt_compute_feedback(coupler):
    """At the end of a GCM step: "esmt_x_tend" = (M(esmt_x / rho) - gcm_x) / gcm_physics_dt, the momentum tendency handed back."""
    _esmt_diagnose(coupler, _esmt_ready(coupler, "esmt_compute_feedback"), ("esmt_u_tend", "esmt_v_tend"), True)


def esmt_pgf(coupler, dt=None, forcing=True):
    """Every CRM step, after the dycore and the sponge layer and before the SGS: pam_amd_esmt_diagnose, then pam_amd_esmt_pgf in place
    on esmt_u and esmt_v with the wavenumbers 1 .. "esmt_kmax"; forcing: "esmt_x_forcing" is applied as well.  Nothing else is
    written.  dt: default the option "crm_dt"."""
    dm = _esmt_ready(coupler, "esmt_pgf")
    lib = capi.load()
    dt = float(coupler.get_option("crm_dt") if dt is None else dt)
    _esmt_diagnose(coupler, dm, None, False)
    P = lambda n: dm.get(n, readonly=True).data_ptr()
    work = dm.get("esmt_workspace")
    with torch.cuda.device(coupler.device):
        check(lib.pam_amd_esmt_pgf(coupler.get_nens(), coupler.get_nx(), coupler.get_ny(), coupler.get_nz(), dm.get("esmt_u").data_ptr(),
                                   dm.get("esmt_v").data_ptr(), P("wvel"), P("density_dry"), P("water_vapor"), P("vertical_midpoint_height"),
                                   P("vertical_cell_dz"), P("esmt_rho_mean"), P("esmt_u_mean"), P("esmt_v_mean"),
                                   P("esmt_u_forcing") if forcing else None, P("esmt_v_forcing") if forcing else None, P("esmt_cos"),
                                   P("esmt_sin"), float(coupler.get_dx()), dt, int(coupler.get_option("esmt_kmax")), work.data_ptr(),
                                   work.numel(), torch.cuda.current_stream(coupler.device).cuda_stream))
