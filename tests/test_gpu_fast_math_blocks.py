"""The scalar building blocks of each arithmetic mode, measured in isolation on the device against double precision
(pt_selfcheck_fast_math, csrc/pt_fast_math_check.inc) — what the per-sample bounds of tests/test_gpu_shade_modes.py and
tests/test_gpu_primitive_modes.py take for granted:
  rcp_, sqrt_, normalize()'s 1 / sqrt over EVERY float bit pattern (normal operands and results): in exact and fma — the IEEE
    sequences — correctly rounded, <= 0.5 ulp, and 1 / sqrt as the reference's inversesqrt forms it, 1.0f / sqrtf(x), <= 1.5 ulp
    (the root's half ulp is up to one ulp of the reciprocal, whose own rounding adds a half); <= 1 ulp in fast, as
    csrc/pt_arith.inc states for v_rcp_f32 / v_rsq_f32 / v_sqrt_f32;
  the sampling's sin / cos of revolutions over EVERY value a draw can return (minstd states 1 .. 2^31 - 2): <= 1.6 ulp above 1e-3
    for the fma mode's ptmath::sincos_rev, as csrc/pt_shade.inc and DESIGN.md state (tests/test_portable_math.py has the host);
  v_sin_f32 / v_cos_f32 (fast): the project states no accuracy, so none is asserted — the measured maximum is printed, stands in
    DESIGN.md's table of arithmetic modes as tau_hw, and is pinned as shade_ref64.TAU_HW, the trig term of the fast bound; the pin
    is checked against the measurement so that the bound cannot rest on a stale figure."""
import numpy as np
import pytest

import shade_ref64 as s64
from cosc_4397_pathtracing_raytracing_project_amd import capi

pytestmark = pytest.mark.gpu
DRAWS = (1, (1 << 31) - 2)  # first state, count


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_reciprocal_and_roots_over_every_float(arith):
    exact_bound = {"rcp": 0.5 + 1e-9, "sqrt": 0.5 + 1e-9, "rsq": 1.5 + 1e-9}  # (the measurement is a double division: 1e-9 of an ulp)
    got = {k: capi.selfcheck_fast_math(k, 0, 1 << 32, arith=arith) for k in ("rcp", "sqrt", "rsq")}
    print(f"BLOCKS {arith}: max ulp over all floats {got}")
    for k, v in got.items():
        assert 0.0 < v <= (1.0 if arith == "fast" else exact_bound[k]), (arith, k, v)


def test_fma_sincos_rev_over_every_draw():
    got = {k: capi.selfcheck_fast_math(k, *DRAWS, arith="fma") for k in ("sin_rev_ulp", "cos_rev_ulp", "sin_rev", "cos_rev", "sin_lobe", "cos_lobe")}
    print(f"BLOCKS fma: sincos_rev over every draw {got}")
    assert 0.0 < got["sin_rev_ulp"] <= 1.6 and 0.0 < got["cos_rev_ulp"] <= 1.6, got
    # 1.6 ulp of a value below 1 is at most 1.6 * 2^-24 absolute; the lobe's angle roughness * u / 4 is rounded to float first
    # (half an ulp of 1/4 revolution = 2^-27 revolutions = 2 pi 2^-27 radians)
    assert max(got["sin_rev"], got["cos_rev"]) <= 1.6 * 2.0 ** -24
    assert max(got["sin_lobe"], got["cos_lobe"]) <= 1.6 * 2.0 ** -24 + 2 * np.pi * 2.0 ** -27


@pytest.mark.parametrize("kind,state,before", [("sin_rev_ulp", 21371167, 1.9675), ("cos_rev_ulp", 579625001, 1.9428)])
def test_fma_sincos_rev_contraction_regression(kind, state, before):
    """The draws that showed it: compiled with contraction on, the fma build formed sincos_rev's reduced argument as
    fma(f, TWO_PI_HI, rl), which counts the head product's rounding error twice — 1.9675 ulp (sin, minstd state 21371167) and
    1.9428 ulp (cos, state 579625001) where the sequence as written gives 0.9675 and 0.9428.  pt_portable_math.h now pins the sequence."""
    got = capi.selfcheck_fast_math(kind, state, 1, arith="fma")
    print(f"BLOCKS fma: {kind} at state {state}: {got:.4f} ulp (was {before})")
    assert 0.0 < got <= 1.6


def test_fast_hardware_sin_cos_is_what_the_shade_bound_was_given():
    got = {k: capi.selfcheck_fast_math(k, *DRAWS, arith="fast") for k in ("sin_rev", "cos_rev", "sin_lobe", "cos_lobe", "sin_rev_ulp", "cos_rev_ulp")}
    print(f"BLOCKS fast: v_sin_f32 / v_cos_f32 over every draw {got}")
    assert all(np.isfinite(v) for v in got.values())
    tau = max(got["sin_rev"], got["cos_rev"], got["sin_lobe"], got["cos_lobe"])
    print(f"BLOCKS fast: tau_hw = {tau:.4g} (pinned {s64.TAU_HW:.4g})")
    assert tau <= s64.TAU_HW  # the pin, not an accuracy claim


def test_refuses_bad_arguments():
    import ctypes as C
    e = C.c_double(0)
    assert capi.lib().pt_selfcheck_fast_math(2, 9, 0, 1, C.byref(e)) != 0 and b"pt_selfcheck_fast_math" in capi.lib().pt_last_error()
    assert capi.lib().pt_selfcheck_fast_math(3, 0, 0, 1, C.byref(e)) != 0
    assert capi.lib().pt_selfcheck_fast_math(2, 0, 0, 1, None) != 0
