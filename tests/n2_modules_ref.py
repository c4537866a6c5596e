"""Plain numpy restatements, in np.longdouble, of the three oldest coupler modules as the reference's headers define them, and the
per-cell tolerances the device, the oracle (C, double) and a numpy-double emulation of the device's summation order are gated at
(tests/test_n2_modules_cells.py; the states and the mutants are in tests/n2_modules_cases.py).

  sponge_layer                      pam_core/modules/sponge_layer.h:65-95
  perturb_temperature               pam_core/modules/perturb_temperature.h:22-61, with the oracle's splitmix64 and int64 seed
  broadcast_initial_gcm_column[_dry_density]   pam_core/modules/broadcast_initial_gcm_column.h

Every restatement takes the double inputs as exact numbers and evaluates the header's formula in extended precision, so what it
returns is, to 2^-64, the real-number result r of that formula on those inputs.  M_PI is the DOUBLE value of pi: the function restated
is the one computed.  The broadcast is a copy, so its restatement works on the uint64 view (a NaN's payload has to arrive).

Sponge layer: the per-cell gate
-------------------------------
u = 2^-53.  For the cell value v of a field on level k of member e: h the exact level mean (0 for wvel, field 3), A the mean of |f|
over the level, tf = dt / time_scale, F the exact factor, r = v + (h - v) F.  Every cell is gated at

    tol = u [ 2 |r|  +  F (ncol + 2) A  +  (|h| + |v|) (4 F + 16 tf) ]

What the double code computes is  v (+) ((h~ (-) v) (x) F~)  with h~ and F~ the computed mean and factor (first order in u throughout):

 * h~ = sum of the ncol products fl(v_c x rho), rho = fl(1 / ncol).  A product carries rho's rounding and its own, 2u; added in ANY
   order an addend passes through at most ncol - 1 additions.  |h~ - h| <= (ncol + 1) u A, gated as (ncol + 2) u A; it reaches the
   result times F.  No order is assumed, on purpose: the same gate holds for the oracle's serial sum, for the device's deal into 16
   slots, and for products contracted into fused multiply-adds (one rounding fewer each).
 * the subtraction h~ (-) v and the product with F~ round once each: 2 u (|h| + |v|) F.
 * F~ = space~ (x) tf~.  tf~ = fl(dt / time_scale) and the product: 2 u F, times (|h| + |v|).  With the line above that is the 4 F.
 * space~ = (cos(M_PI x rel) + 1) / 2.  rel <= 1 carries three roundings (two differences of heights, one division) and M_PI x rel a
   fourth: the cosine's argument, at most pi, is off by 4 pi u = 12.6 u at most and |sin| <= 1 passes that on; a cosine good to 2 ulp
   adds 2u, the addition of 1 (a sum in [0, 2]) another 2u, the halving is exact: (12.6 + 2 + 2) / 2 = 8.3 u absolute.  (Counting the
   four roundings as 4u, without the factor pi, gives 8u.)  The figure is doubled: 16 u, absolute on the space factor, so 16 u tf on F.
   It is an ABSOLUTE term: on the bottom sponge level rel = 1 and the exact F is ~ 4e-33 tf, while a cosine one ulp off leaves 5e-17 tf;
   that level is therefore gated by tol like every other and not bit for bit against the input.
 * the final addition: u |r|.  The gate carries 2 |r|; the second u absorbs the second-order terms dropped above.

Levels below the sponge must equal the input bit for bit (no tolerance: the kernel must not touch them).

perturb_temperature: the per-cell gate
--------------------------------------
The perturbed cells (levels k < nz/4) are gated at (2 ncol + 10) u |r|, valid for positive temperatures, with
r = (T + rnd m s) h1 / h2, h1 and h2 the level means before and after, s = (nl - k) / nl.

 * rnd = 2 U - 1 with U = (z >> 11) 2^-53 is exact in binary: z >> 11 has 53 bits, 2U - 1 is a multiple of 2^-52 of magnitude <= 1.
 * p = rnd (x) m (x) s~ with s~ = fl((nl - k) / nl): 3 u |p|; v~ = T (+) p: u |v|.  With |p| <= 0.13 |v| (30 K on 230 K at the worst)
   the perturbed cell is good to 1.4 u |v|.
 * h1~: ncol products fl(T_c x rho), 2u each, summed in any order, (ncol - 1) u: (ncol + 1) u h1 -- all addends are positive, so the
   sum of magnitudes IS the sum.  That is where positive temperatures are needed.
 * h2~: the same on the perturbed cells, which carry their own 1.4 u: (ncol + 2.4) u h2.
 * v~ (x) h1~ (/) h2~: two more roundings, and v~'s 1.4 u.

Sum: (ncol + 1) + (ncol + 2.4) + 1.4 + 2 = 2 ncol + 6.8, gated as 2 ncol + 10.  Levels k >= nz/4 must equal the input bit for bit.
(With ncol = 1 the rescale restores the cell: h1 = T, h2 = v, r = T.)
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
M_PI = LD(float(np.pi))          # the double value of pi, held in extended precision
WFLD = 3                         # wvel relaxes towards zero (sponge_layer.h:34,:77)
MOD_NS = 16                      # slots of the device's horizontal sums (pam_amd/csrc/modules_kernels.hip)

_MASK = (1 << 64) - 1
_GOLDEN, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def splitmix64_next(state):
    """One step of splitmix64 on Python integers: (new state, output).  Known answers: state 0 -> 0xE220A8397B1DCDAF first."""
    state = (state + _GOLDEN) & _MASK
    z = state
    z = ((z ^ (z >> 30)) * _M1) & _MASK
    z = ((z ^ (z >> 27)) * _M2) & _MASK
    return state, z ^ (z >> 31)


def splitmix64_ints(seed):
    """the first output of a generator whose state is `seed`, elementwise: int64 (or uint64) array -> uint64 array.  A negative seed
    wraps as the C cast (uint64_t)seed does."""
    with np.errstate(over="ignore"):
        z = np.asarray(seed).astype(np.int64).astype(np.uint64) + np.uint64(_GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        return z ^ (z >> np.uint64(31))


def unit_ints(seed):
    """the 53-bit integers the unit doubles are made of: U = unit_ints * 2^-53"""
    return splitmix64_ints(seed) >> np.uint64(11)


# ---- sponge_layer -----------------------------------------------------------------------------------------------------------------

def sponge_factor(zint, zmid, num_layers, tf):
    """F (nz, nens) in longdouble, zero below the sponge (sponge_layer.h:91-93); tf = dt / time_scale in longdouble"""
    nz, nens = zmid.shape
    zi, zm = zint.astype(LD), zmid.astype(LD)
    F = np.zeros((nz, nens), dtype=LD)
    kbot = nz - 1 - (num_layers - 1)
    for k in range(kbot, nz):
        rel = (zi[nz] - zm[k]) / (zi[nz] - zm[kbot])
        F[k] = (np.cos(M_PI * rel) + 1) / 2 * tf
    return F


def stack(fields):
    """coupler fields (dict as for the oracle) -> (nf, nz, ny, nx, nens) in the reference's order: rho_d, u, v, w, T, tracers..."""
    return np.concatenate([np.stack([fields[k] for k in ("density_dry", "uvel", "vvel", "wvel", "temp")]), fields["tracers"]])


def unstack(X):
    f = dict(zip(("density_dry", "uvel", "vvel", "wvel", "temp"), (np.ascontiguousarray(x) for x in X[:5])))
    f["tracers"] = np.ascontiguousarray(X[5:])
    return f


def sponge(X, zint, zmid, dt, num_layers=5, time_scale=60.0, mutant=None):
    """X (nf, nz, ny, nx, nens) double -> dict(r=, tol=, F=, h=, A=), all (nf, nz, ny, nx, nens)-broadcastable longdouble but tol, which
    is double.  `mutant` names one deliberate error (tests/n2_modules_cases.py: SPONGE_MUTANTS); tol is always that of the true
    formula."""
    nf, nz, ny, nx, nens = X.shape
    ncol = ny * nx
    tf = LD(dt) / LD(time_scale)
    v = X.astype(LD)
    F = sponge_factor(zint, zmid, num_layers, tf)                                  # (nz, nens)
    h = v.mean(axis=(2, 3), dtype=LD)                                              # (nf, nz, nens)
    h[WFLD] = 0
    A = np.abs(v).mean(axis=(2, 3), dtype=LD)
    Fb, hb, Ab = F[None, :, None, None, :], h[:, :, None, None, :], A[:, :, None, None, :]
    r = v + (hb - v) * Fb
    tol = U * (2 * np.abs(r) + Fb * (ncol + 2) * Ab + (np.abs(hb) + np.abs(v)) * (4 * Fb + 16 * tf))
    out = dict(r=r, tol=tol.astype(np.float64), F=F, h=h, A=A, sponge=slice(nz - num_layers, nz))
    if mutant is None:
        return out
    Fm, hm = F.copy(), h.copy()
    flat = v.reshape(nf, nz, ncol, nens)
    if mutant == "member0_heights":
        Fm = np.repeat(sponge_factor(zint[:, :1], zmid[:, :1], num_layers, tf), nens, axis=1)
    elif mutant == "factor_from_level_above":      # level k takes the factor of k + 1; the top one that of the model top, rel = 0
        Fm[nz - num_layers:nz - 1] = F[nz - num_layers + 1:]
        Fm[nz - 1] = tf
    elif mutant == "factor_halved":
        Fm = F / 2
    elif mutant == "w_to_its_mean":
        hm[WFLD] = v[WFLD].mean(axis=(1, 2), dtype=LD)
    elif mutant == "mean_drops_ragged_tail":       # only the cells of full rounds of 16
        hm = flat[:, :, :MOD_NS * (ncol // MOD_NS)].sum(axis=2, dtype=LD) / ncol
        hm[WFLD] = 0
    elif mutant == "mean_drops_slot_15":
        keep = np.arange(ncol) % MOD_NS != MOD_NS - 1
        hm = flat[:, :, keep].sum(axis=2, dtype=LD) / ncol
        hm[WFLD] = 0
    elif mutant == "tracer_means_swapped":
        hm[[5, 6]] = h[[6, 5]]
    elif mutant == "mean_from_member_plus_64":
        hm = h[:, :, (np.arange(nens) + 64) % nens]
    elif mutant not in ("last_tracer_skipped", "one_cell_1e-9"):
        raise KeyError(mutant)
    rm = v + (hm[:, :, None, None, :] - v) * Fm[None, :, None, None, :]
    if mutant == "last_tracer_skipped":
        rm[nf - 1] = v[nf - 1]
    if mutant == "one_cell_1e-9":
        # the (field, level, member) of the sponge with the smallest non-zero magnitude; its largest cell, off by 1e-9 of itself
        sp = out["sponge"]
        mag = np.abs(r[:, sp]).max(axis=(2, 3))
        mag = np.where(mag > 0, mag, np.inf)
        f, k, e = np.unravel_index(np.argmin(mag), mag.shape)
        j, i = np.unravel_index(np.argmax(np.abs(r[f, sp][k, :, :, e])), (ny, nx))
        rm[f, nz - num_layers + k, j, i, e] *= 1 + LD(1e-9)
        out["cell"] = (f, nz - num_layers + k, j, i, e)
    out["r"] = rm
    return out


def sponge_slot_emulation(X, zint, zmid, dt, num_layers=5, time_scale=60.0):
    """The device's order in numpy double, no contraction: cell c goes to slot c % 16, every slot adds its products v x fl(1/ncol) in
    ascending order, the 16 slot sums are added in ascending order from 0.0; the factor as the header writes it, glibc's cosine."""
    nf, nz, ny, nx, nens = X.shape
    ncol = ny * nx
    out = X.copy()
    flat = out.reshape(nf, nz, ncol, nens)
    r_nx_ny = 1.0 / ncol
    time_factor = dt / time_scale
    kbot = nz - 1 - (num_layers - 1)
    pi = float(np.pi)
    for k in range(kbot, nz):
        slots = np.zeros((MOD_NS, nf, nens))
        for c in range(ncol):
            slots[c % MOD_NS] += flat[:, k, c, :] * r_nx_ny
        h = np.zeros((nf, nens))
        for s in range(MOD_NS):
            h += slots[s]
        h[WFLD] = 0.0
        rel_dist = (zint[nz] - zmid[k]) / (zint[nz] - zmid[kbot])
        factor = (np.cos(pi * rel_dist) + 1) / 2 * time_factor
        vk = flat[:, k].copy()
        flat[:, k] = vk + (h[:, None, :] - vk) * factor[None, None, :]
    return out


def worst_ratio(got, ref):
    """max over the cells of |got - r| / tol, and where; a cell with tol = 0 (an exact zero that must stay one) counts as 0 when it is
    met and as inf when it is not"""
    err = np.abs(got.astype(LD) - ref["r"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(ref["tol"] > 0, err / ref["tol"], np.where(err > 0, np.inf, 0.0))
    w = np.unravel_index(np.argmax(q), q.shape)
    return float(q[w]), tuple(int(x) for x in w)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- perturb_temperature ------------------------------------------------------------------------------------------------------------

def perturb_seeds(ids, nz, ny, nx, mutant=None):
    """the int64 seeds (nl, ny, nx, nens) of perturb_temperature.h:46, with the oracle's 64-bit arithmetic"""
    nl, nens = nz // 4, len(ids)
    idv = np.asarray(ids, dtype=np.int64)
    if mutant == "id_of_member_before":
        idv = np.roll(idv, 1)
    k, j, i, e = np.meshgrid(np.arange(nl, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64),
                             np.arange(nens), indexing="ij")
    if mutant == "seed_without_level":
        return idv[e] * nl * ny * nx + j * nx + i
    if mutant == "seed_member_fastest":
        return ((k * ny + j) * nx + i) * nens + idv[e]
    return idv[e] * nl * ny * nx + k * ny * nx + j * nx + i


def perturb(T, ids, magnitude=0.1, mutant=None):
    """T (nz, ny, nx, nens) double -> dict(r=, tol=, nl=, ratio=): r longdouble (levels >= nl are the input), tol double (zero there:
    bits), ratio = hmean1 / hmean2 (nl, 1, 1, nens)"""
    nz, ny, nx, nens = T.shape
    nl, ncol = nz // 4, ny * nx
    r = T.astype(LD)
    tol = np.zeros(T.shape)
    out = dict(r=r, tol=tol, nl=nl)
    if nl == 0:
        return out
    rnd = unit_ints(perturb_seeds(ids, nz, ny, nx, mutant)).astype(LD) * LD(2.0 ** -53) * 2 - 1
    rnd = np.maximum(np.minimum(rnd, LD(1)), LD(-1))
    k = np.arange(nl)
    s = (nl - (k + 1 if mutant == "scaling_of_level_above" else k)).astype(LD) / nl
    t0 = r[:nl]
    h1 = t0.mean(axis=(1, 2), keepdims=True, dtype=LD)
    if mutant == "hmean1_of_next_member":
        h1 = np.roll(h1, -1, axis=3)
    v = t0 + rnd * LD(magnitude) * s[:, None, None, None]
    h2 = v.mean(axis=(1, 2), keepdims=True, dtype=LD)
    true = v * h1 / h2
    out["ratio"] = (h1 / h2).astype(np.float64)
    r[:nl] = v * h2 / h1 if mutant == "rescale_inverted" else true
    if mutant is None:
        tol[:nl] = ((2 * ncol + 10) * U * np.abs(true)).astype(np.float64)
    return out


def perturb_serial_emulation(T, ids, magnitude=0.1):
    """the oracle's (and the device's: one thread walks a level of a member) serial double arithmetic in numpy, no contraction"""
    nz, ny, nx, nens = T.shape
    nl, ncol = nz // 4, ny * nx
    out = T.copy()
    if nl == 0:
        return out
    flat = out.reshape(nz, ncol, nens)
    r_nx_ny = 1.0 / ncol
    rnd = (unit_ints(perturb_seeds(ids, nz, ny, nx)).astype(np.float64) * (1.0 / 9007199254740992.0)) * 2. - 1.
    rnd = np.maximum(np.minimum(rnd, 1.0), -1.0).reshape(nl, ncol, nens)
    for k in range(nl):
        h1, h2 = np.zeros(nens), np.zeros(nens)
        for c in range(ncol):
            h1 += flat[k, c] * r_nx_ny
        scaling = (nl - float(k)) / nl
        for c in range(ncol):
            flat[k, c] = flat[k, c] + rnd[k, c] * magnitude * scaling
            h2 += flat[k, c] * r_nx_ny
        for c in range(ncol):
            flat[k, c] = flat[k, c] * h1 / h2
    return out


# ---- broadcast_initial_gcm_column ---------------------------------------------------------------------------------------------------

def broadcast(crm_bits, gcm_bits, nfields):
    """crm_bits: list of six (nz, ny, nx, nens) uint64 arrays, gcm_bits: six (nz, nens); the first nfields (6, or 1: the dry-density
    variant) are overwritten with the column, the rest returned as they came"""
    out = [c.copy() for c in crm_bits]
    for f in range(nfields):
        out[f][...] = gcm_bits[f][:, None, None, :]
    return out
