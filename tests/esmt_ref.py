"""Explicit scalar momentum transport for 2-D CRMs (Tulich 2015): the numpy restatement of the contract (include/pam_amd_modules.h at
pam_amd_esmt_pgf), operation for operation.  TEST INFRASTRUCTURE ONLY.

numpy's element-wise float64 arithmetic is IEEE and never contracted and no numpy reduction takes part (the level means are
msa_ref.level_mean, a loop over the cells in the slot order; the sums of the transform are loops in the order of the contract), so the
device bodies are held to this file bit for bit.  Everything is vectorised over the members only where the contract leaves the order
free (different members, levels and cells never meet).

A case is a dict:
  fields    wvel, density_dry, water_vapor, esmt_u, esmt_v, (nz,1,nx,nens)
  zmid, dz  (nz,nens)
  force_u, force_v   (nz,nens) or None
  cos, sin  the tables (nx)
  dx, dt, kmax
  skip_v    True: the call is made without v_mean (the C ABI's NULL), so esmt_v takes no pressure force
  gcm_u, gcm_v (nz,nens) or None, gcm_dt: what diagnose turns into tendencies"""
import numpy as np

import msa_ref
from sgs_ref import same_bits      # noqa: F401

TWO_PI = 6.283185307179586
SCALARS = ("esmt_u", "esmt_v")
RD, RV = "density_dry", "water_vapor"
MUTANTS = ("nyquist_scale", "sine_sign", "a_c_swapped", "centred_end_gradient", "k2_not_doubled", "plain_mean")


def shape_id(shape):
    return "%dx1x%d-e%d" % shape


def tables(nx):
    """C[j] = cos((2 pi j) / nx), S[j] = sin((2 pi j) / nx): what the init forms on the host (the kernels take them as given)"""
    x = (TWO_PI * np.arange(nx, dtype=np.float64)) / np.float64(nx)
    return np.cos(x), np.sin(x)


def level_mean(f, mutant=None):
    """M(f)(k,e) of a (nz,1,nx,nens) field, in MSA's slot order"""
    nz, ny, nx, nens = f.shape
    if mutant == "plain_mean":
        return f.reshape(nz, nx, nens).mean(axis=1)
    return msa_ref.level_mean(f.reshape(nz, ny * nx, nens))


def set_scalars(rho_d, rho_v, src_u, src_v):
    rho = rho_d + rho_v
    return rho * src_u[:, None, None, :], rho * src_v[:, None, None, :]


def diagnose(case, feedback=False, mutant=None):
    """-> rho_mean, u_mean, v_mean, and tend_u / tend_v where the case holds gcm_u / gcm_v"""
    F = case["fields"]
    with np.errstate(all="ignore"):
        rho = F[RD] + F[RV]
        out = dict(rho_mean=level_mean(rho, mutant), u_mean=level_mean(F["esmt_u"] / rho, mutant), v_mean=level_mean(F["esmt_v"] / rho, mutant))
        for x in "uv":
            gcm = case.get("gcm_" + x)
            if gcm is not None:
                d = out[x + "_mean"] - gcm if feedback else gcm - out[x + "_mean"]
                out["tend_" + x] = d / np.float64(case["gcm_dt"])
    return out


def gradient(X, z, mutant=None):
    G = np.empty_like(X)
    G[0] = (X[1] - X[0]) / (z[1] - z[0])
    G[-1] = (X[-1] - X[-2]) / (z[-1] - z[-2])
    if mutant == "centred_end_gradient":      # a mirrored ghost level: half the one-sided slope
        G[0] = (X[1] - X[0]) / (2.0 * (z[1] - z[0]))
        G[-1] = (X[-1] - X[-2]) / (2.0 * (z[-1] - z[-2]))
    if X.shape[0] > 2:
        G[1:-1] = (X[2:] - X[:-2]) / (z[2:] - z[:-2])
    return G


def force(w, rho_mean, means, z, h, C, S, dx, kmax, mutant=None):
    """T_X (nz,nx,nens) for every X of `means` (a dict of (nz,nens) level means) from w (nz,nx,nens)"""
    nz, nx, nens = w.shape
    k1 = np.float64(TWO_PI) / (np.float64(nx) * np.float64(dx))
    s, s_nyq = np.float64(2.0) / np.float64(nx), np.float64(1.0) / np.float64(nx)
    with np.errstate(all="ignore"):
        a, c = np.zeros((nz, nens)), np.zeros((nz, nens))
        a[1:] = 1.0 / (h[1:] * (z[1:] - z[:-1]))
        c[:-1] = 1.0 / (h[:-1] * (z[1:] - z[:-1]))
        if mutant == "a_c_swapped":
            a, c = c, a
        G = {x: gradient(X, z, mutant) for x, X in means.items()}
        T = {x: np.zeros((nz, nx, nens)) for x in means}
        for m in range(1, kmax + 1):
            idx = (m * np.arange(nx)) % nx
            nyq = 2 * m == nx
            kap = np.float64(m) * k1
            k2 = kap * kap
            b = (a + c) + k2
            wc, ws = np.zeros((nz, nens)), np.zeros((nz, nens))
            for i in range(nx):
                wc = wc + w[:, i, :] * C[idx[i]]
                if not nyq:
                    ws = ws + w[:, i, :] * S[idx[i]]
            wc = (s_nyq if nyq and mutant != "nyquist_scale" else s) * wc
            ws = s * ws
            cp, den = np.empty((nz, nens)), np.empty((nz, nens))
            den[0] = b[0]
            cp[0] = -c[0] / den[0]
            for k in range(1, nz):
                den[k] = b[k] + a[k] * cp[k - 1]
                cp[k] = -c[k] / den[k]
            fac = (k2 if mutant == "k2_not_doubled" else 2.0 * k2) / rho_mean
            for x in means:
                for comp, tab, sign in ((wc, C, 1.0),) + (() if nyq else ((ws, S, -1.0 if mutant == "sine_sign" else 1.0),)):
                    R = (rho_mean * G[x]) * comp
                    d, psi = np.empty((nz, nens)), np.empty((nz, nens))
                    d[0] = R[0] / den[0]
                    for k in range(1, nz):
                        d[k] = (R[k] + a[k] * d[k - 1]) / den[k]
                    psi[nz - 1] = d[nz - 1]
                    for k in range(nz - 2, -1, -1):
                        psi[k] = d[k] - cp[k] * psi[k + 1]
                    That = fac * psi
                    T[x] = T[x] + sign * (That[:, None, :] * tab[idx][None, :, None])
    return T


def pgf(case, mutant=None, means=None):
    """diagnose on the state at entry, then the force: -> {esmt_u, esmt_v}"""
    F = case["fields"]
    D = means or diagnose(case, mutant=mutant)
    nz, _, nx, nens = F["wvel"].shape
    dt, kmax = np.float64(case["dt"]), int(case["kmax"])
    given = {"u": D["u_mean"]} if case.get("skip_v") else {"u": D["u_mean"], "v": D["v_mean"]}
    T = force(F["wvel"].reshape(nz, nx, nens), D["rho_mean"], given, case["zmid"], case["dz"], case["cos"], case["sin"], case["dx"], kmax,
              mutant) if kmax > 0 else {}
    out = {}
    with np.errstate(all="ignore"):
        rho = F[RD] + F[RV]
        for x in "uv":
            f = case.get("force_" + x)
            old = F["esmt_" + x]
            if x in T and f is not None:
                inc = dt * T[x].reshape(old.shape) + (dt * f)[:, None, None, :]
            elif x in T:
                inc = dt * T[x].reshape(old.shape)
            elif f is not None:
                inc = np.broadcast_to((dt * f)[:, None, None, :], old.shape)
            else:
                out["esmt_" + x] = old.copy()
                continue
            out["esmt_" + x] = old + rho * inc
    return out


def members(case, idx):
    """the case on a selection of members (members are independent)"""
    sub = dict(case, fields={n: np.ascontiguousarray(a[..., idx]) for n, a in case["fields"].items()})
    for n in ("zmid", "dz", "force_u", "force_v", "gcm_u", "gcm_v"):
        if case.get(n) is not None:
            sub[n] = np.ascontiguousarray(case[n][:, idx])
    return sub


def results_differ(x, y, nan_by_place=False):
    """names of what differs bitwise between two results; nan_by_place: a NaN equals any NaN at the same place"""
    bad = []
    for n in y:
        a, b = np.ascontiguousarray(x[n]), np.ascontiguousarray(y[n])
        if a.shape != b.shape:
            bad.append(n)
        elif nan_by_place:
            na, nb = np.isnan(a), np.isnan(b)
            if not (np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])):
                bad.append(n)
        elif not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
            bad.append(n)
    return bad


class RefBackend:
    def diagnose(self, case, feedback=False):
        return diagnose(case, feedback)

    def run(self, case):
        return pgf(case)
