"""CPU-only: every literal of the
reference's generated matrices that the hot path uses (dynamics/awfl/TransformMatrices.h: sten_to_coefs<5,5> :970,
coefs_to_gll_lower<5,2> :1132, weno_lower_sten_to_coefs<3,3,3> :1218, coefs_to_tv<3> :188, coefs_to_tv<5> :871,
get_gll_points<9> :4113, get_gll_weights<9> :4126) against the constants this repository derives independently from
exact rationals (tools/gen_constants.py -> awfl_constants.h).  The reference's values are read from its headers by
`extract` (tests/golden/extract_reference.py) and recorded as data in tests/golden/reference_extract.json; the tests compare
with that record.  This pins the constants of the oracle and of the HIP kernels to the reference itself."""
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_extract.json")
TV5_TERMS = {(1, 1): "AWFL_TV5_A1A1", (2, 2): "AWFL_TV5_A2A2", (1, 3): "AWFL_TV5_A1A3", (3, 3): "AWFL_TV5_A3A3",
             (2, 4): "AWFL_TV5_A2A4", (4, 4): "AWFL_TV5_A4A4"}


def _function_body(text, signature):
    i = text.index(signature)
    j = text.index("\n  }\n", i)
    return text[i:j]


def _matrix(text, signature, shape):
    body = _function_body(text, signature)
    a = np.full(shape, np.nan)
    for m in re.finditer(r"rslt\(([\d,]+)\)=(-?[\d.]+(?:e-?\d+)?)", body):
        a[tuple(int(x) for x in m.group(1).split(","))] = float(m.group(2))
    assert not np.isnan(a).any(), signature
    return a


def _ours(name, shape=None):
    hdr = open(os.path.join(ROOT, "pam_amd", "csrc", "awfl_constants.h")).read()
    assert hdr == open(os.path.join(ROOT, "oracle", "awfl_constants.h")).read()      # kernels and oracle share the values
    m = re.search(r"#define " + name + r" (.*?)\n(?=#define|/\*|\n#endif)", hdr, flags=re.S)
    txt = m.group(1).replace("\\\n", " ")
    vals = [float(v) for v in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?", txt)]
    return np.array(vals).reshape(shape) if shape else vals[0]


def _recorded():
    return json.load(open(GOLDEN))["constants"]


def test_generated_constants_equal_the_reference_literals():
    ref = _recorded()
    m = {k: np.array(v) for k, v in ref["matrices"].items()}
    assert np.abs(m["sten_to_coefs_5x5"] - _ours("AWFL_STEN_TO_COEFS_INIT", (5, 5))).max() <= 1e-16
    assert np.abs(m["coefs_to_gll_lower_5x2"] - _ours("AWFL_COEFS_TO_GLL_INIT", (5, 2))).max() <= 1e-16
    assert np.abs(m["weno_lower_sten_to_coefs_3x3x3"] - _ours("AWFL_WENO_LOWER_INIT", (3, 3, 3))).max() <= 1e-16
    assert np.abs(m["gll_points_9"] - _ours("AWFL_GLL9_PTS_INIT", (9,))).max() <= 1e-16
    assert np.abs(m["gll_weights_9"] - _ours("AWFL_GLL9_WTS_INIT", (9,))).max() <= 1e-16
    # total-variation quadratic forms: coefficient of each monomial in the reference expression
    tv3, tv5 = ref["tv3_coefs"], ref["tv5_coefs"]
    assert tv3["1,1"] == 1.0 and abs(tv3["2,2"] - _ours("AWFL_TV3_A2A2")) <= 1e-15
    for (i, j), name in TV5_TERMS.items():
        assert abs(tv5["%d,%d" % (i, j)] - _ours(name)) <= 1e-13 * max(1.0, abs(_ours(name))), (i, j)
    # no other monomial appears in the reference's quartic form
    assert set(ref["tv5_monomials"]) == {"%d,%d" % ij for ij in TV5_TERMS}


def test_weno_ideal_weights_and_scalar_constants_equal_the_reference():
    """wenoSetIdealSigma<5> (WenoLimiter.h:37-43), the acoustic speed cs = 350 (Dycore.h:335), hs = (ord+1)/2 (Dycore.h:23)."""
    ref = _recorded()
    assert ref["weno5_sigma"] == _ours("AWFL_WENO_SIGMA")
    assert ref["weno5_idl"] == list(_ours("AWFL_WENO_IDL_INIT", (4,)))
    assert ref["dycore_cs"] == 350
    dev = open(os.path.join(ROOT, "pam_amd", "csrc", "awfl_device.h")).read()
    assert "const double cs = 350.0" in dev and "constexpr int HS = 3;" in dev
    assert ref["dycore_hs_is_half_ord_plus_one"]      # ord = 5 -> 3 halo / ghost cells


KESSLER_LITERALS = ["36.34", "0.1364", "3.8", "17.27", "2.2", "0.875", "4093.", "1.6", "124.9", "0.2046", "0.525",
                    "2550000.", "540000.", "273.", "36.", "0.001", "0.8", "1.e-10"]


def test_kessler_and_module_literals_appear_in_reference_oracle_and_kernels():
    """Numeric literals of the Kessler scheme (physics/micro/kessler/Microphysics.h:346-457) and of the sponge layer
    defaults: each must be present in the reference text, in the oracle restatement and in the HIP kernels (a typo guard;
    the arithmetic itself is covered by the oracle-vs-HIP parity tests)."""
    ref = _recorded()
    ora = open(os.path.join(ROOT, "oracle", "awfl_oracle.c")).read()
    hip = open(os.path.join(ROOT, "pam_amd", "csrc", "kessler_device.h")).read()      # the bodies of the Kessler kernels
    for lit in KESSLER_LITERALS:
        pat = re.escape(lit.rstrip(".")) + r"(?![\d])"
        assert lit in ref["kessler_literals_found"], ("reference", lit)
        assert re.search(pat, ora), ("oracle", lit)
        assert re.search(pat, hip), ("kernels", lit)
    from pam_amd.micro import Microphysics
    for name in ("R_d", "cp_d", "cp_v", "R_v", "p0", "grav"):      # the scheme's constants, Microphysics.h:66-71
        assert ref["kessler_constants"][name] == getattr(Microphysics, name), name
    assert ref["sponge_num_layers"] == 5 and ref["sponge_time_scale"] == 60


def extract(ref_root):
    """what the tests of this module record of the reference tree at `ref_root` (tests/golden/extract_reference.py stores it)"""
    ref = open(os.path.join(ref_root, "dynamics", "awfl", "TransformMatrices.h")).read()
    mats = {"sten_to_coefs_5x5": ("void sten_to_coefs(SArray<FP,2,5,5> &rslt)", (5, 5)),
            "coefs_to_gll_lower_5x2": ("void coefs_to_gll_lower(SArray<FP,2,5,2> &rslt)", (5, 2)),
            "weno_lower_sten_to_coefs_3x3x3": ("void weno_lower_sten_to_coefs(SArray<FP,3,3,3,3> &rslt)", (3, 3, 3)),
            "gll_points_9": ("void get_gll_points(SArray<FP,1,9> &rslt)", (9,)),
            "gll_weights_9": ("void get_gll_weights(SArray<FP,1,9> &rslt)", (9,))}
    out = {"matrices": {k: _matrix(ref, sig, shape).tolist() for k, (sig, shape) in mats.items()}}
    tv3 = _function_body(ref, "FP coefs_to_tv(SArray<FP,1,3> &a)")
    tv5 = _function_body(ref, "FP coefs_to_tv(SArray<FP,1,5> &a)")

    def coef(body, i, j):
        m = re.search(r"(-?[\d.]+)_fp\*\(?a\(%d\)\*a\(%d\)\)?" % (i, j), body)
        return float(m.group(1)) if m else 0.0
    out["tv3_coefs"] = {"%d,%d" % ij: coef(tv3, *ij) for ij in ((1, 1), (2, 2))}
    out["tv5_coefs"] = {"%d,%d" % ij: coef(tv5, *ij) for ij in TV5_TERMS}
    out["tv5_monomials"] = sorted(set("%s,%s" % ij for ij in re.findall(r"a\((\d)\)\*a\((\d)\)", tv5)))
    wl = open(os.path.join(ref_root, "dynamics", "awfl", "WenoLimiter.h")).read()
    blk = wl[wl.index("} else if (ord == 5) {"):wl.index("} else if (ord == 7) {")]
    out["weno5_sigma"] = float(re.search(r"sigma = ([\d.]+)_fp", blk).group(1))
    out["weno5_idl"] = [float(x) for x in re.findall(r"idl\(\d\) = ([\d.]+)_fp", blk)]
    dy = open(os.path.join(ref_root, "dynamics", "awfl", "Dycore.h")).read()
    out["dycore_cs"] = int(re.search(r"real constexpr cs = (\d+);", dy).group(1))
    out["dycore_hs_is_half_ord_plus_one"] = bool(re.search(r"static constexpr hs\s*=\s*\(ord\+1\)/2;", dy))
    mp = open(os.path.join(ref_root, "physics", "micro", "kessler", "Microphysics.h")).read()
    out["kessler_literals_found"] = [lit for lit in KESSLER_LITERALS if re.search(re.escape(lit.rstrip(".")) + r"(?![\d])", mp)]
    out["kessler_constants"] = {name: float(re.search(name + r"\s*=\s*([\d.e+]+)\s*;", mp).group(1))
                                for name in ("R_d", "cp_d", "cp_v", "R_v", "p0", "grav")}
    sp = open(os.path.join(ref_root, "pam_core", "modules", "sponge_layer.h")).read()
    out["sponge_num_layers"] = int(re.search(r"num_layers\s*=\s*(\d+);", sp).group(1))
    out["sponge_time_scale"] = float(re.search(r"time_scale\s*=\s*([\d.]+)", sp).group(1))
    return out
