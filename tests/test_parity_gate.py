"""CPU-only: the parity gate itself (tests/parity_gate.py) against the oracle, on every named case of tests/test_gpu_parity.py
(built by tests/parity_cases.py without a device).

 * The floor gate is never looser than the curve it replaces, and every floor is finite and positive where its field is not zero.
 * It is not tighter than pure noise: a fourth twin with another seed -- one more oracle run that differs from the unperturbed one
   only by one ulp of T -- passes it in every case.
 * It catches what the curve lets through: the oracle with a gravity constant off by 1e-11 (a kernel with a slightly wrong
   constant) fails it in four cases, where the curve catches two of them; off by 1e-12, it fails in three, where the curve catches
   none."""
import copy
import functools

import numpy as np
import pytest

from parity_cases import CASES, named_case
from parity_gate import compare, gates, is_tight, perturbed_twins, tol_noise_fields, worst_errors


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, oracle output, sub-steps, floor) of a named case"""
    c = named_case(name)
    base = c.inputs()
    nsub = c.run(base)
    return c, base, nsub, c.floor(base=base)


def _noise_keys(c):
    return [k for k in ["uvel", "vvel", "wvel"] + list(c.names) if not is_tight(k)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_floor_gate_is_within_the_curve_and_floors_are_positive(name):
    c, base, nsub, floor = _case(name)
    curve = tol_noise_fields(nsub, c.gate_factor)
    gate = gates(base, c.names, nsub, c.gate_factor, floor)
    for k in _noise_keys(c):
        assert 0.0 <= gate[k] <= curve, (k, gate[k], curve)
    for k, e in floor.items():
        field = base["tracers"][c.names.index(k)] if k in c.names else base[k.split("_elementwise")[0]]
        assert np.isfinite(e), (k, e)
        if np.any(field):
            assert e > 0.0, (k, "a nonzero field the twins left bit-identical")


@pytest.mark.parametrize("name", sorted(CASES))
def test_independent_twin_passes_the_floor_gate(name):
    """one more twin, from a seed the floor did not use, stays within the gate: the gate does not fail pure noise.  Fields that are
    identically zero in the oracle are left out: there the gate is 0 (the device keeps them exactly zero, as the oracle does, since
    it runs the unperturbed input), while a T perturbed cell by cell breaks the symmetry that keeps them zero (v of the 3x3x3 grid)."""
    c, base, nsub, floor = _case(name)
    twin = perturbed_twins(c.fields, 1)[0]
    assert not np.array_equal(twin["temp"], c.fields["temp"])
    c.run(twin)
    gate = gates(base, c.names, nsub, c.gate_factor, floor)
    worst = worst_errors(twin, base, c.names)
    for k, e in worst.items():
        if gate[k] > 0.0:
            assert e <= gate[k], (k, e, gate[k], floor.get(k))


def _mutant(name, rel):
    """the oracle of case `name` with grav scaled by (1 + rel): a kernel with a slightly wrong constant"""
    c, base, nsub, floor = _case(name)
    consts = dict(c.consts, grav=c.consts["grav"] * (1.0 + rel))
    f = c.inputs()
    assert c.run(f, consts) == nsub
    return f


@pytest.mark.parametrize("rel,name", [(1e-11, "3d_nt1_vapour_limited_nens64"), (1e-11, "c3_grid_32x1x60_L60_nt4"),
                                      (1e-11, "3d_nt10_perens_A_p3"), (1e-11, "2d_nt4_stretched_A"),
                                      (1e-12, "3d_nt1_vapour_limited_nens64"), (1e-12, "3d_nt10_perens_A_p3"),
                                      (1e-12, "2d_nt4_stretched_A")])
def test_wrong_gravity_constant_fails_the_floor_gate(rel, name):
    c, base, nsub, floor = _case(name)
    with pytest.raises(AssertionError):
        compare(_mutant(name, rel), base, c.names, nsub, factor=c.gate_factor, floor=floor)


def test_injected_perturbation_fails_the_floor_gate():
    """as test_gpu_parity's check of the curve: 1e-10 relative in ONE field turns the case red, also under the floor gate"""
    c, base, nsub, floor = _case("3d_nt4_stretched_B")
    compare(base, base, c.names, nsub, factor=c.gate_factor, floor=floor)
    for k in ("uvel", "wvel", "temp"):
        bad = copy.deepcopy(base)
        bad[k] = bad[k] * (1.0 + 1.0e-10)
        with pytest.raises(AssertionError):
            compare(bad, base, c.names, nsub, floor=floor)
    bad = copy.deepcopy(base)
    bad["tracers"][1] = bad["tracers"][1] * (1.0 + 1.0e-10)
    with pytest.raises(AssertionError):
        compare(bad, base, c.names, nsub, floor=floor)


def test_zero_field_must_stay_zero():
    """2-D v is identically zero in the oracle: under the floor gate any nonzero v fails, however small"""
    c, base, nsub, floor = _case("2d_nt1_uniform_A")
    assert not np.any(base["vvel"])
    assert gates(base, c.names, nsub, floor=floor)["vvel"] == 0.0
    bad = copy.deepcopy(base)
    bad["vvel"][0, 0, 0, 0] = 1e-30
    with pytest.raises(AssertionError):
        compare(bad, base, c.names, nsub, floor=floor)


def test_without_a_floor_the_gate_is_the_curve():
    """floor=None (smoke()) keeps the gate as it was: 1e-12 for rho_d, T, vapour, the curve for every other field"""
    c, base, nsub, floor = _case("3d_nt4_stretched_B")
    gate = gates(base, c.names, nsub)
    for k, g in gate.items():
        assert g == (1e-12 if is_tight(k) else tol_noise_fields(nsub)), k
