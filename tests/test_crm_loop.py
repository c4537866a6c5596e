"""The composed CRM loop on the CPU, no device (tests/crm_loop_ref.py is the chain): the chain run through the emulated device bodies
against the chain of the numpy restatements, bit for bit; every scheme of the stack acts on the seeded state; three wrong orders of the
calls and one wrong tracer flag each leave the gate of the free-running GPU comparison; and the conditions of that gate, on the reference
alone, for every named stack."""
import numpy as np
import pytest

import crm_loop_ref as loop
import ice1m_ref
import lsforcing_ref
from parity_gate import FLOOR_K, TOL_TIGHT, is_tight

STACK_NAMES = tuple(loop.STACKS)
_RUNS = {}


def _traced(name):
    """the chain's run of a stack with the state after every call and the ice scheme's census, once per stack and shared"""
    if name not in _RUNS:
        k = loop.stack(name)
        trace, census = [], {}
        state = loop.run_state(k, trace=trace, census=census)
        _RUNS[name] = (k, state, trace, census)
    return _RUNS[name]


def _emulated_kernels():
    """the g++-built device bodies behind the interface of the restatements.  Without a harness, and so left on numpy: the stored-heating
    step (pam_amd_radiation_forced has a restatement in plugins_ref and no emulated body).  The dycore and the sponge layer are the oracle
    in both chains"""
    from esmt_harness import EmuBackend as Esmt
    from grayrad_emu_harness import EmuBackend as Lw
    from grayrad_sw_emu_harness import EmuBackend as Sw
    from hd_emu_harness import EmuBackend as Hd
    from ice1m_harness import EmuBackend as Ice
    from lsforcing_harness import EmuBackend as Ls
    from sgs_moist_emu_harness import EmuBackend as Moist
    from sgs_tke_harness import EmuBackend as Tke
    from surface_emu_harness import EmuBackend as Surface
    from test_sgs_horizontal import EmuBackend as Horizontal
    lw, sw, hd, ice, ls, moist, tke, sfc, hor, esmt = Lw(), Sw(), Hd(), Ice(), Ls(), Moist(), Tke(), Surface(), Horizontal(), Esmt()

    def ls_run(case):
        out, inc = ls.run(case, with_inc=True)
        return out, inc

    def esmt_run(case):
        return esmt.diagnose(case), esmt.run(case)

    return dict(lw=lw.run, sw=sw.run, ls=ls_run, esmt=esmt_run, surface=sfc.run, hd=hd.run, tke_coefficients=tke.coefficients,
                smag_coefficients=moist.coefficients, horizontal=lambda case, tk, tkh: hor.run(dict(case, tk=tk, tkh=tkh)),
                diffuse=moist.diffuse, ice=ice.run)


@pytest.mark.parametrize("name", ["full3d_flat", "full2d_esmt"])
def test_chain_through_the_emulated_bodies_equals_the_numpy_chain_bit_for_bit(name):
    """every call of every step: each entry the DataManager would hold has the same bits in both chains.  full3d_flat is the TKE stack;
    full2d_esmt adds the two paths it does not take, ESMT and the moist Smagorinsky coefficients"""
    k, _, want, _ = _traced(name)
    got = []
    loop.run_state(k, trace=got, kernels=_emulated_kernels())
    assert len(got) == len(want) == k.steps * len(loop.order(k))
    for i, ((call, _, a), (call_w, _, b)) in enumerate(zip(got, want)):
        assert call == call_w
        bad = [n for n in b if not ice1m_ref.same_bits(np.ascontiguousarray(a[n]), np.ascontiguousarray(b[n]))]
        assert bad == [], (i // len(loop.order(k)), call, bad)
    print("%s: %d calls, %d entries each, all bits equal" % (name, len(want), len(want[-1][2])))


@pytest.mark.parametrize("name", STACK_NAMES)
def test_every_scheme_acts(name):
    """on the seeded state no part of the stack idles: the run holds cloud ice and snow, both surface precipitation rates, tk > 0 and
    tkh > tk, surface fluxes and a slab that moved, shortwave heating, a wind the Coriolis term turned, a tracer the dycore's limiter
    acted on, and the melting, freezing, riming and sublimation branches of the ice scheme, each taken at least once"""
    k, state, trace, census = _traced(name)
    S = state.S
    assert S["cloud_ice"].max() > 0 and S["precip_ice"].max() > 0
    assert S["precl"].max() > 0 and S["preci"].max() > 0
    assert (S["tk"] > 0).any() and (S["tkh"] > S["tk"]).any()
    assert np.abs(S["sfc_shf"] + S["sfc_lhf"]).max() > 0
    assert not ice1m_ref.same_bits(S["sfc_temp"], k.S0["sfc_temp"])
    assert np.abs(S["rad_sw_heating"]).max() > 0
    # both radiation steps occurred: the computing one wrote the outputs, the stored-heating one temp alone
    wrote = [set(allowed) for call, allowed, _ in trace if call == "radiation"]
    assert {"rad_olr"} <= wrote[0] and wrote[1] == {"temp"}
    # the Coriolis term: the large-scale forcing of the first step with and without it
    first = loop.start(k)
    loop.step(first, k, until="sponge_layer")
    with_f = lsforcing_ref.ls_forcing(loop.ls_case(k, first.S))
    without = lsforcing_ref.ls_forcing(loop.ls_case(k, first.S, coriolis=False))
    assert np.abs(with_f["vvel"] - without["vvel"]).max() > 1.0e-4 and np.abs(with_f["uvel"] - without["uvel"]).max() > 1.0e-5
    # the limiter: the first dycore step with every positivity flag off differs in a tracer
    a, b = loop.start(k), loop.start(k, positive=[False] * len(k.names))
    for s in (a, b):
        loop.step(s, k, until="dycore")
    limited = [n for n in k.names if not ice1m_ref.same_bits(a.S[n], b.S[n])]
    assert limited, "the limiter acted on no tracer"
    branches = dict(melting=census["melt_by_ice"] + census["melt_by_heat"], freezing=census["freeze_by_liquid"] + census["freeze_by_heat"],
                    riming=census["riming"], sublimation=census["snow_limit_all"] + census["snow_limit_half"] + census["snow_limit_rate"])
    assert all(v > 0 for v in branches.values()), branches
    print("%s: limiter on %s; ice branches %s" % (name, limited, branches))


def _swapped(k, call, after=None, before=None):
    calls = [c for c in loop.order(k) if c != call]
    at = calls.index(after) + 1 if after is not None else calls.index(before)
    return tuple(calls[:at] + [call] + calls[at:])


MUTANTS = ("surface_after_closure", "sponge_before_dycore", "radiation_after_micro", "tke_not_positive")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_gate_sees_a_wrong_order_and_a_wrong_flag(mutant):
    """full3d_flat with the surface fluxes after the closure, the sponge layer before the dycore, the radiation after the microphysics, or
    the tracer tke not positive-definite in the dycore: each differs from the chain by more than the free-running gate in a quantity"""
    k = loop.stack("full3d_flat")
    base, held, floor = loop.floors(k)
    gate = loop.gates(k, base, floor)
    kw = {"surface_after_closure": dict(calls=_swapped(k, "surface_fluxes", after="sgs")),
          "sponge_before_dycore": dict(calls=_swapped(k, "sponge_layer", before="dycore")),
          "radiation_after_micro": dict(calls=_swapped(k, "radiation", after="micro")),
          "tke_not_positive": dict(positive=[n != "tke" and p for n, p in zip(k.names, k.positive)])}[mutant]
    state = loop.run_state(k, **kw)
    worst = loop.errors(k, loop.to_fields(k, state.S), state.S, base, held)
    beyond = {n: "%.1e > %.1e" % (worst[n], gate[n]) for n in worst if worst[n] > gate[n]}
    print(mutant, beyond)
    assert beyond, worst


@pytest.mark.parametrize("name", STACK_NAMES)
def test_conditions_of_the_free_running_gate_hold_on_the_reference(name):
    """parity_gate.noise_floor through the whole chain (three twins with one ulp of noise in temp): rho_d, temp and the vapour of the twins
    stay within TOL_TIGHT / 10, and for every noise quantity FLOOR_K x floor stays at or below a tenth of its cap (1e-8 for the winds and
    the tracers other than vapour, 1e-10 for the column outputs), so the cap is never what passes a case.  The floors (seed 0):

      full3d_flat (10,5,6,3), 3 steps: rho_d 1.8e-15, temp 1.6e-15, vapour 1.4e-14; u 6.1e-14, v 2.2e-14, w 4.7e-14, cloud_liquid 5.5e-14,
        cloud_ice 8.3e-14, rain 2.1e-15, snow 2.6e-15, tke 7.0e-15; precl 2.1e-15, preci 1.1e-14, sfc_temp 0, rad_olr 5.5e-15,
        rad_lw_down_sfc 8.6e-14, rad_lw_up_sfc 0, rad_sw_down_sfc and rad_sw_up_sfc 1.3e-13, rad_sw_up_top 1.2e-14
      full3d_members (8,5,5,65), 2 steps: rho_d 2.5e-15, temp 1.9e-15, vapour 2.0e-14; u 4.9e-14, v 2.2e-14, w 1.1e-13, cloud_liquid
        6.4e-14, cloud_ice 1.1e-13, rain 1.8e-15, snow 6.8e-14, tke 2.2e-14; precl 1.6e-15, preci 1.3e-14, sfc_temp 0, rad_olr 6.5e-16,
        rad_lw_down_sfc 1.4e-15, rad_lw_up_sfc and the shortwave fluxes 0 (the second step applies the stored heating)
      full2d_esmt (10,1,9,66), 3 steps: rho_d 2.5e-15, temp 2.0e-15, vapour 1.9e-14; u 4.1e-14, v 2.2e-15, w 7.3e-14, cloud_liquid 7.3e-14,
        cloud_ice 1.8e-13, rain 2.0e-14, snow 3.8e-14, esmt_u 4.5e-15, esmt_v 3.4e-15; precl 3.2e-14, preci 4.5e-14, sfc_temp 0, rad_olr
        6.1e-15, rad_lw_down_sfc 1.6e-13, rad_lw_up_sfc 0, rad_sw_down_sfc and rad_sw_up_sfc 2.6e-13, rad_sw_up_top 2.1e-14

    (a cold layer under the sounding carries the snow to the ground: without it preci is 1e-21 m/s of leaked mixing with a floor of
    3e-12, tests/crm_loop_ref.py)"""
    k = loop.stack(name)
    base, held, floor = loop.floors(k)
    print(name, k.shape, {n: float("%.2g" % v) for n, v in floor.items()})
    for n, v in floor.items():
        if is_tight(n):
            assert v <= TOL_TIGHT / 10, (n, v)
        else:
            cap = loop.CAP_COLUMN if n in loop.COLUMN_OUTPUTS else loop.CAP_NOISE
            assert FLOOR_K * v <= cap / 10, (n, v, cap)
    assert set(loop.COLUMN_OUTPUTS) <= set(floor) and set(k.names) <= set(floor)
