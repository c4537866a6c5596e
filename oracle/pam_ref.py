"""ctypes binding of the reference itself, compiled serially against the YAKL stand-in.   TEST INFRASTRUCTURE ONLY.

`make -C oracle` builds oracle/_ref/libpam_ref.so from the reference's own headers (oracle/ref/ref_harness.cpp + the stand-in
oracle/ref/YAKL.h) when the reference tree is present.  This module loads only that library -- never a path in the reference
tree -- so GPU tests may import it wherever oracle/_ref/ travelled.  `available()` says whether it is there.

`RefDycore` has the call shapes of `awfl_oracle.OracleDycore`, so a test can run the same sequence on either checker.
Two switches of the stand-in are set here:
  * allocation fill: NaN by default (a read of memory the reference never wrote shows in the outputs); `alloc_fill(zero=True)`
    for the one path that depends on fresh memory being zero;
  * the D1 replay: the vertical boundary kernel of Dycore::halo_exchange (label D1_REPLAY_LABEL) runs twice, which makes its
    ghost read-after-write order-independent.  `replay_count()` counts the replays.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libpam_ref.so")
# YAKL_AUTO_LABEL of the boundary-condition parallel_for in halo_exchange (file:line of the reference header)
D1_REPLAY_LABEL = "awfl/Dycore.h:662"
_LIB = None
_DP = C.POINTER(C.c_double)


def available():
    return os.path.exists(LIB_PATH)


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not available():
        raise FileNotFoundError(LIB_PATH + " is not built (make -C oracle with the reference tree present)")
    lib = C.CDLL(LIB_PATH)
    lib.pam_ref_set_alloc_fill.argtypes = [C.c_int]
    lib.pam_ref_set_replay_label.argtypes = [C.c_char_p]
    lib.pam_ref_replay_count.restype = C.c_long
    lib.pam_ref_dycore_create.restype = C.c_void_p
    lib.pam_ref_dycore_create.argtypes = [C.c_int] * 5 + [C.c_double] * 2 + [_DP, C.c_char_p, C.c_char_p, C.c_char_p, _DP]
    lib.pam_ref_dycore_destroy.argtypes = [C.c_void_p]
    lib.pam_ref_dycore_set_grav_balance.argtypes = [C.c_void_p, C.c_int]
    lib.pam_ref_dycore_get_option.restype = C.c_double
    lib.pam_ref_dycore_get_option.argtypes = [C.c_void_p, C.c_char_p]
    lib.pam_ref_dycore_declare_hydrostatic.restype = C.c_int
    lib.pam_ref_dycore_declare_hydrostatic.argtypes = [C.c_void_p] + [_DP] * 6 + [C.POINTER(_DP)]
    lib.pam_ref_dycore_compute_time_step.restype = C.c_double
    lib.pam_ref_dycore_compute_time_step.argtypes = [C.c_void_p] + [_DP] * 6 + [C.c_double]
    lib.pam_ref_dycore_time_step.restype = C.c_int
    lib.pam_ref_dycore_time_step.argtypes = [C.c_void_p] + [_DP] * 6 + [C.c_double, _DP]
    lib.pam_ref_dycore_read.restype = C.c_long
    lib.pam_ref_dycore_read.argtypes = [C.c_void_p, C.c_char_p, _DP, C.c_long]
    lib.pam_ref_set_replay_label(D1_REPLAY_LABEL.encode())
    _LIB = lib
    return lib


def set_replay_label(label):
    """None switches the replay off (mode A then reads the stale ghost, as the reference does in serial order)."""
    load().pam_ref_set_replay_label(label.encode() if label else None)


def replay_count():
    return load().pam_ref_replay_count()


def reset_replay_count():
    load().pam_ref_reset_replay_count()


def alloc_fill(zero):
    load().pam_ref_set_alloc_fill(int(bool(zero)))


def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_DP)


class RefDycore:
    """The reference `Dycore` on a reference `PamCoupler`, with OracleDycore's constructor and methods.

    Tracer names: `names` if given, else water_vapor at idWV and tracer_<i> elsewhere (the dycore reads only the flags and
    finds water vapour by name)."""

    def __init__(self, nens, nx, ny, nz, xlen, ylen, dz, tracer_positive, tracer_adds_mass, idWV, consts=None, names=None):
        self.lib = load()
        self.nens, self.nx, self.ny, self.nz = nens, nx, ny, nz
        self.nt = len(tracer_positive)
        if names is None:
            names = ["water_vapor" if t == idWV else "tracer_%d" % t for t in range(self.nt)]
        assert len(names) == self.nt and names[idWV] == "water_vapor"
        self.names = list(names)
        self._dz = np.ascontiguousarray(np.broadcast_to(np.asarray(dz, dtype=np.float64).reshape(nz, -1), (nz, nens)))
        pos = bytes(bytearray(int(bool(x)) for x in tracer_positive))
        mass = bytes(bytearray(int(bool(x)) for x in tracer_adds_mass))
        cp = None
        if consts is not None:
            self._consts = np.array([consts[k] for k in ("R_d", "cp_d", "R_v", "cp_v", "p0", "grav")], dtype=np.float64)
            cp = _p(self._consts)
        self.h = self.lib.pam_ref_dycore_create(nens, nx, ny, nz, self.nt, float(xlen), float(ylen), _p(self._dz),
                                                "\n".join(self.names).encode(), pos, mass, cp)
        if not self.h:
            raise RuntimeError("reference Dycore::init failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.pam_ref_dycore_destroy(self.h)
            self.h = None

    def option(self, key):
        return self.lib.pam_ref_dycore_get_option(self.h, key.encode())

    def set_grav_balance(self, flag):
        self.lib.pam_ref_dycore_set_grav_balance(self.h, int(bool(flag)))

    def _read(self, name, shape):
        out = np.empty(shape)
        n = self.lib.pam_ref_dycore_read(self.h, name.encode(), _p(out), out.size)
        if n != out.size:
            raise KeyError(name)
        return out

    @property
    def variable_gravity(self):
        return self._read("variable_gravity", (self.nz, self.nens))

    @property
    def hy_dens_cells(self):
        return self._read("hy_dens_cells", (self.nz, self.nens))

    @property
    def hy_pressure_cells(self):
        return self._read("hy_pressure_cells", (self.nz, self.nens))

    @property
    def vert_sten_to_coefs(self):
        return self._read("vert_sten_to_coefs", (self.nz + 2, 5, 5, self.nens))

    @property
    def vert_weno_recon_lower(self):
        return self._read("vert_weno_recon_lower", (self.nz + 2, 3, 3, 3, self.nens))

    def _f(self, fields):
        return [_p(fields[k]) for k in ("density_dry", "uvel", "vvel", "wvel", "temp", "tracers")]

    def declare_current_profile_as_hydrostatic(self, fields, gcm=None):
        arr = None
        if gcm is not None:
            self._gcm = [np.ascontiguousarray(gcm[k], dtype=np.float64) for k in
                         ("gcm_density_dry", "gcm_temp", "gcm_water_vapor", "gcm_cloud_water", "gcm_cloud_ice")]
            arr = (_DP * 5)(*[_p(a) for a in self._gcm])
        if self.lib.pam_ref_dycore_declare_hydrostatic(self.h, *self._f(fields), arr) != 0:
            raise RuntimeError("reference declare_current_profile_as_hydrostatic failed")

    def compute_time_step(self, fields, cfl=0.8):
        return self.lib.pam_ref_dycore_compute_time_step(self.h, *self._f(fields), float(cfl))

    def time_step(self, fields, crm_dt):
        out = C.c_double(0)
        n = self.lib.pam_ref_dycore_time_step(self.h, *self._f(fields), float(crm_dt), C.byref(out))
        if n < 0:
            raise RuntimeError("reference timeStep failed")
        return n, out.value


def _load_modules(lib):
    if getattr(lib, "_modules_bound", False):
        return lib
    lib.pam_ref_coupler_create.restype = C.c_void_p
    lib.pam_ref_coupler_create.argtypes = [C.c_int] * 5 + [C.c_double] * 2 + [_DP, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.pam_ref_coupler_destroy.argtypes = [C.c_void_p]
    lib.pam_ref_coupler_set_real.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    lib.pam_ref_coupler_set_int.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.pam_ref_coupler_set_string.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    lib.pam_ref_coupler_register.restype = C.c_int
    lib.pam_ref_coupler_register.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    for f in (lib.pam_ref_coupler_write, lib.pam_ref_coupler_read):
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_char_p, _DP, C.c_long]
    lib.pam_ref_coupler_run.restype = C.c_int
    lib.pam_ref_coupler_run.argtypes = [C.c_void_p, C.c_char_p, _DP, _DP]
    lib.pam_ref_supercell_init.restype = C.c_int
    lib.pam_ref_supercell_init.argtypes = [C.c_int, _DP] + [C.c_double] * 3 + [_DP] * 6
    lib._modules_bound = True
    return lib


class RefCoupler:
    """A reference `pam::PamCoupler` of (nz,ny,nx,nens) on the grid zint (nz+1,nens), tracers (name, positive, adds_mass) registered
    in the given order.  Entries are written / read by name as numpy arrays; `run(module)` calls the reference's module of that
    name (sponge_layer, compute_gcm_forcing_tendencies, apply_gcm_forcing_tendencies, broadcast_initial_gcm_column[_dry_density],
    saturation_adjustment, surface_friction_init, compute_surface_friction, kessler_init, kessler_timeStep)."""

    def __init__(self, nz, ny, nx, nens, xlen, ylen, zint, tracers=()):
        self.lib = _load_modules(load())
        self.shape = (nz, ny, nx, nens)
        self._zint = np.ascontiguousarray(np.broadcast_to(np.asarray(zint, dtype=np.float64).reshape(nz + 1, -1), (nz + 1, nens)))
        names = "\n".join(t[0] for t in tracers).encode()
        pos = bytes(bytearray(int(bool(t[1])) for t in tracers))
        mass = bytes(bytearray(int(bool(t[2])) for t in tracers))
        self.h = self.lib.pam_ref_coupler_create(nens, nx, ny, nz, len(tracers), float(xlen), float(ylen), _p(self._zint), names,
                                                 pos, mass)
        if not self.h:
            raise RuntimeError("reference coupler creation failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.pam_ref_coupler_destroy(self.h)
            self.h = None

    def set_option(self, key, value):
        if isinstance(value, str):
            self.lib.pam_ref_coupler_set_string(self.h, key.encode(), value.encode())
        elif isinstance(value, (int, np.integer)) and not isinstance(value, bool):
            self.lib.pam_ref_coupler_set_int(self.h, key.encode(), int(value))
        else:
            self.lib.pam_ref_coupler_set_real(self.h, key.encode(), float(value))

    def register(self, name, dims):
        d = (C.c_int * len(dims))(*dims)
        if self.lib.pam_ref_coupler_register(self.h, name.encode(), len(dims), d) != 0:
            raise RuntimeError("register " + name)

    def write(self, name, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if self.lib.pam_ref_coupler_write(self.h, name.encode(), _p(a), a.size) != a.size:
            raise KeyError(name)

    def read(self, name, shape):
        out = np.empty(shape)
        if self.lib.pam_ref_coupler_read(self.h, name.encode(), _p(out), out.size) != out.size:
            raise KeyError(name)
        return out

    def run(self, module, a=None, b=None):
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (a, b)]
        rc = self.lib.pam_ref_coupler_run(self.h, module.encode(), *[None if x is None else _p(x) for x in arrs])
        if rc == -2:
            raise ValueError("unknown module " + module)
        if rc != 0:
            raise RuntimeError("reference " + module + " failed")


def supercell_init(zint, consts):
    """standalone supercell_init on zint (nz+1,) -> (rho_d, uvel, vvel, wvel, temp, rho_v), each (nz,)"""
    lib = _load_modules(load())
    z = np.ascontiguousarray(zint, dtype=np.float64)
    nz = len(z) - 1
    out = [np.zeros(nz) for _ in range(6)]
    if lib.pam_ref_supercell_init(nz, _p(z), consts["R_d"], consts["R_v"], consts["grav"], *[_p(a) for a in out]) != 0:
        raise RuntimeError("reference supercell_init failed")
    return out
