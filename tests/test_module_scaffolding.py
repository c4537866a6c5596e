"""The module entry points without a HIP device: every one whose device check was spelled on its own (a literal, or a concatenation in
place) returns PAM_AMD_ENOGPU with exactly "<who>: no HIP device available (this library has no CPU path)" once its arguments pass.
The sizes are valid and every pointer points at real host memory; nothing is dereferenced before the device check but the pointer
tables.  Skipped where a device is present."""
import ctypes as C

import numpy as np
import pytest

from pam_amd import capi

ENOGPU = -2
TAIL = ": no HIP device available (this library has no CPU path)"


def _calls(lib):
    buf = np.zeros(64)
    p = buf.ctypes.data

    def table(n):
        return (C.c_void_p * n)(*[p] * n)
    return buf, [
        ("sponge_layer", lambda: lib.pam_amd_sponge_layer(2, 4, 1, 8, 6, table(6), p, p, 1.0, 5, 60.0, None, None)),
        ("kessler", lambda: lib.pam_amd_kessler_time_step(2, 4, 1, 8, p, p, p, p, p, p, p, 1.0, 287.0, 461.0, 1003.0, 1.0e5, p, None, 0, None)),
        ("compute_gcm_forcing_tendencies", lambda: lib.pam_amd_gcm_forcing_compute(2, 4, 1, 8, table(10), table(10), table(14), 1200.0, None)),
        ("broadcast_initial_gcm_column", lambda: lib.pam_amd_broadcast_initial_gcm_column(2, 4, 1, 8, 6, table(6), table(6), None)),
        ("perturb_temperature", lambda: lib.pam_amd_perturb_temperature(2, 4, 1, 8, p, p, 0.1, None)),
        ("supercell_init", lambda: lib.pam_amd_supercell_init(8, p, 287.0, 461.0, 9.8, p, p, p, p, p, p, None)),
        ("saturation_adjustment", lambda: lib.pam_amd_saturation_adjustment(2, 4, 1, 8, p, p, p, p, 0, None, 461.0, 1003.0, 1859.0, 4188.0, None)),
    ]


def test_entry_points_name_themselves_when_there_is_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    lib = capi.load()
    buf, calls = _calls(lib)
    for who, call in calls:
        assert call() == ENOGPU, who
        assert lib.pam_amd_awfl_last_error() == (who + TAIL).encode(), who
    assert not buf.any()
