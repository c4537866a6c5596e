"""CPU-only census of the anisotropic named cases (tests/parity_cases.py, ANISOTROPIC_CASES): what each of them must be for a
kernel that confuses dy with dx, or that gets the y direction wrong only where there is flow along y, to fail it.  Conditions on the
oracle alone -- no kernel is run here -- stated and asserted:

 * dx != dy, the ratio outside [0.8, 1.25]; nx != ny, both at least 5.
 * Sensitivity to the spacing: the oracle on the case's inputs with ylen replaced by ny * dx -- exactly what a dy -> dx confusion
   computes -- departs from the true result by at least 1000 times the case's gate (tests/parity_gate.py) in every gated field:
   rho_d, u, v, w, T (max-norm and element-wise) and every tracer that is not identically zero.
 * Sensitivity to y flow: max|v| of the inputs is at least max|u| / 2, and the oracle's largest y face flux of every tracer is at
   least a tenth of its largest x face flux (compute_tendencies(..., want_fluxes=True) on the inputs).
 * Limiter across y (dry_air cases): the limiter scales a y face flux of water vapour out of a cell that is not on an x edge of the
   carved air.  What the limiter did is read off the oracle by running the same stage with dt = 0, where it cannot act.
 * The record of the gap: every named case from before these is isotropic with the shear along x, one test per case."""
import numpy as np
import pytest

from parity_cases import ANISOTROPIC_CASES, CASES, ISOTROPIC_CASES, named_case
from parity_gate import gates, worst_errors
from test_parity_gate import _case

SPACING_MARGIN = 1000.0       # the dy -> dx result must miss the gate by this factor


def test_the_anisotropic_cases_exist_in_both_orders_of_the_ratio():
    ratios = [named_case_dims(n)[1] / named_case_dims(n)[0] for n in ANISOTROPIC_CASES]
    assert len(ANISOTROPIC_CASES) >= 8 and min(ratios) < 0.8 and max(ratios) > 1.25
    assert any(r <= 0.25 or r >= 4.0 for r in ratios), "one strong ratio"
    flows = {CASES[n][6].get("flow", "x") for n in ANISOTROPIC_CASES}
    assert {"y", "diag"} <= flows


def named_case_dims(name):
    kw = CASES[name][6]
    dx = kw.get("dxy", 500.0)
    return dx, kw.get("dy", dx)


@pytest.mark.parametrize("name", ISOTROPIC_CASES)
def test_earlier_named_case_is_isotropic_with_the_shear_along_x(name):
    nens, nx, ny, nz, tr, zint, kw, mode_a, nsteps = CASES[name]
    dx, dy = named_case_dims(name)
    assert dx == dy and kw.get("flow", "x") == "x", name


@pytest.mark.parametrize("name", ANISOTROPIC_CASES)
def test_grid_is_anisotropic(name):
    c = named_case(name)
    nens, nx, ny, nz = c.dims
    assert nx != ny and min(nx, ny) >= 5
    assert c.xlen == nx * c.dx and c.ylen == ny * c.dy
    assert not 0.8 <= c.dy / c.dx <= 1.25, (c.dx, c.dy)
    for t, n in enumerate(c.names):
        assert np.any(c.fields["tracers"][t]), (n, "a tracer the builder left empty")


@pytest.mark.parametrize("name", ANISOTROPIC_CASES)
def test_dy_taken_for_dx_misses_the_gate_by_three_orders_in_every_field(name):
    c, base, nsub, floor = _case(name)
    nens, nx, ny, nz = c.dims
    slip = c.inputs()
    c.run(slip, ylen=ny * c.dx)
    gate = gates(base, c.names, nsub, c.gate_factor, floor)
    worst = worst_errors(slip, base, c.names)
    print(name, {k: "%.1e (gate %.1e)" % (worst[k], gate[k]) for k in sorted(worst)})
    for k, g in gate.items():
        assert g > 0.0, (k, "identically zero in the oracle: nothing to gate")
        assert worst[k] >= SPACING_MARGIN * g, (k, worst[k], g)


def _first_stage_fluxes(c, dt):
    """the oracle's face fluxes (x, y, z; state and tracers, after the limiter) of the first stage on the case's inputs"""
    f = c.inputs()
    o = c.oracle()
    o.declare_current_profile_as_hydrostatic(f)
    if dt is None:
        dt = o.compute_time_step(f)
    st, trc = o.convert_coupler_to_dynamics(f)
    seed = trc[:, 3:-3, 3:-3, 3:-3, :].copy()
    _, _, fl = o.compute_tendencies(st, trc, seed, dt, want_fluxes=True)
    return fl, seed


@pytest.mark.parametrize("name", ANISOTROPIC_CASES)
def test_flow_along_y_is_as_strong_as_along_x(name):
    c = named_case(name)
    assert c.flow in ("y", "diag")
    u, v = np.abs(c.fields["uvel"]).max(), np.abs(c.fields["vvel"]).max()
    assert v >= 0.5 * u and v >= 5.0, (u, v)
    fl, _ = _first_stage_fluxes(c, None)
    for t, n in enumerate(c.names):
        fx, fy = np.abs(fl[0][5 + t]).max(), np.abs(fl[1][5 + t]).max()
        print(name, n, "largest x / y face flux %.3e / %.3e" % (fx, fy))
        assert fy >= 0.1 * fx > 0.0, (n, fx, fy)


@pytest.mark.parametrize("name", [n for n in ANISOTROPIC_CASES if CASES[n][6].get("dry_air")])
def test_limiter_acts_across_y_away_from_the_x_edges(name):
    c = named_case(name)
    nens, nx, ny, nz = c.dims
    wv = c.idwv
    lim, seed = _first_stage_fluxes(c, None)
    raw, _ = _first_stage_fluxes(c, 0.0)           # mass_out = 0: the limiter scales nothing
    for d in range(3):                             # dt enters the stage through the limiter alone
        assert np.array_equal(lim[d][:5], raw[d][:5])
    fy, ry = lim[1][5 + wv], raw[1][5 + wv]        # (nz, ny + 1, nx, nens): face j is the lower y face of cell j
    assert (fy != ry).any()
    # the donor of a scaled face: the cell below it where the flux is positive, the one above where it is negative
    scaled_up, scaled_dn = (fy != ry) & (ry > 0), (fy != ry) & (ry < 0)
    donor = np.zeros((nz, ny, nx, nens), dtype=bool)
    donor |= scaled_up[:, 1:]
    donor |= scaled_dn[:, :ny]
    wet = seed[wv] > 0.0
    on_x_edge = (wet != np.roll(wet, 1, axis=2)) | (wet != np.roll(wet, -1, axis=2))
    on_y_edge = (wet != np.roll(wet, 1, axis=1)) | (wet != np.roll(wet, -1, axis=1))
    n = int((donor & ~on_x_edge & on_y_edge).sum())
    print(name, "cells whose y flux of vapour the limiter scaled: %d, of them on a y edge and on no x edge: %d" % (donor.sum(), n))
    assert n > 0
