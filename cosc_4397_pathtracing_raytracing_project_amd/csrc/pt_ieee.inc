// pt_ieee.inc — guarded IEEE square root / reciprocal / quotient sequences (namespace ieee), included by pt_kernels.hip
// inside ptk::<arith>::(anonymous); pt_ieee_check.inc holds the device self-check.
// Correctly rounded square root / reciprocal / quotient at about 60 % of the price of the compiler's expansions — same
// results, bit for bit.  The compiler's expansions have to work for every input; three to seven of their 11 (divide) / 16
// (sqrt) instructions — all of the half-rate kind — only serve inputs a path tracer does not see: v_div_scale / v_div_fmas /
// v_div_fixup rescale operands whose quotient could leave the normal range and patch up zeros, infinities and NaNs; the
// sqrt expansion pre-scales inputs below 2^-96, post-scales the result and restores 0 / inf / NaN with a class test.  When
// EVERY active lane of the wave has operands inside a range where those instructions are the identity (one integer
// compare per operand and a scalar branch), what remains is executed:
//   sqrt   s = v_sqrt_f32(x); the neighbours s -/+ 1 ulp; residuals fma(-s', s, x); pick as the expansion does
//   a / b  r = v_rcp_f32(b), one Newton step on r, q = a r, two residual corrections of q — the expansion's FMA chain, with a
//          plain FMA where v_div_fmas (which is an FMA unless v_div_scale set VCC) stood
// otherwise the wave runs the compiler's expansion.  Identity by construction inside the range (it is the same instruction
// sequence); pt_selfcheck_ieee verifies it on the device against `__builtin_sqrtf`, `1.0f / x` and `a / b` for all 2^32 bit
// patterns of x and for 2^33 operand pairs (tests/test_gpu_ieee_ops.py).
namespace ieee {
PT_DEV bool every_lane(bool ok) { return ballot(!ok) == 0ull; }
// |v| in [2^-47, 2^47): the exponents of numerator and denominator differ by less than 96, so v_div_scale leaves both as they
// are (VCC = 0, v_div_fmas is a plain FMA) and the quotient is a normal number — by construction, not only by test (round 3's
// [2^-60, 2^60] relied on the scaled path giving the same result, which the device self-check confirmed but nothing proved)
PT_DEV bool div_range(float v) { return ((__float_as_uint(v) & 0x7fffffffu) - 0x28000000u) < (0x57000000u - 0x28000000u); }
// x in [2^-94, 2^60): above the expansion's pre-scaling threshold (2^-96), finite; the root lies in [2^-47, 2^30), inside div_range
PT_DEV bool sqrt_range(float x) { return (__float_as_uint(x) - 0x10800000u) < (0x5d800000u - 0x10800000u); }
PT_DEV float sqrt_core(float x) {
#pragma clang fp contract(off)
  const float s = __builtin_amdgcn_sqrtf(x);
  const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
  const float rd = __builtin_fmaf(-dn, s, x), ru = __builtin_fmaf(-up, s, x);
  float r = rd <= 0.0f ? dn : s;
  r = ru > 0.0f ? up : r;
  return r;
}
PT_DEV float rcp_core(float b) {  // the refined reciprocal the quotients of one denominator share
#pragma clang fp contract(off)
  const float r = __builtin_amdgcn_rcpf(b);
  const float e = __builtin_fmaf(-b, r, 1.0f);
  return __builtin_fmaf(e, r, r);
}
PT_DEV float quot_core(float a, float b, float r) {
#pragma clang fp contract(off)
  float q = a * r;
  const float e2 = __builtin_fmaf(-b, q, a);
  q = __builtin_fmaf(e2, r, q);
  const float e3 = __builtin_fmaf(-b, q, a);
  return __builtin_fmaf(e3, r, q);
}
PT_DEV float sqrt(float x) {
  if (every_lane(sqrt_range(x))) return sqrt_core(x);
  return __builtin_sqrtf(x);
}
PT_DEV float div(float a, float b) {
  if (every_lane(div_range(a) && div_range(b))) return quot_core(a, b, rcp_core(b));
  return a / b;
}
PT_DEV float rcp(float b) {
  if (every_lane(div_range(b))) return quot_core(1.0f, b, rcp_core(b));
  return 1.0f / b;
}
// 1 / sqrt(x) as the reference forms it: two correctly rounded operations.  One range test covers both.
PT_DEV float rcp_sqrt(float x) {
  if (every_lane(sqrt_range(x))) {
    const float s = sqrt_core(x);
    return quot_core(1.0f, s, rcp_core(s));
  }
  return 1.0f / __builtin_sqrtf(x);
}
// (a1 / b, a2 / b) and (1/x, 1/y, 1/z): one range test, and the two quotients of one denominator share its reciprocal
PT_DEV void div2(float a1, float a2, float b, float& q1, float& q2) {
  if (every_lane(div_range(a1) && div_range(a2) && div_range(b))) {
    const float r = rcp_core(b);
    q1 = quot_core(a1, b, r), q2 = quot_core(a2, b, r);
    return;
  }
  q1 = a1 / b, q2 = a2 / b;
}
// (a.x, a.y, a.z) / b.  (Zero numerators stay outside the guarded range: the correction chain turns -0 / b into +0 — found by the
// self-check.)
PT_DEV void div3(float& x, float& y, float& z, float b) {
  if (every_lane(div_range(x) && div_range(y) && div_range(z) && div_range(b))) {
    const float r = rcp_core(b);
    x = quot_core(x, b, r), y = quot_core(y, b, r), z = quot_core(z, b, r);
    return;
  }
  x = x / b, y = y / b, z = z / b;
}
PT_DEV void rcp3(float x, float y, float z, float& rx, float& ry, float& rz) {
  if (every_lane(div_range(x) && div_range(y) && div_range(z))) {
    rx = quot_core(1.0f, x, rcp_core(x)), ry = quot_core(1.0f, y, rcp_core(y)), rz = quot_core(1.0f, z, rcp_core(z));
    return;
  }
  rx = 1.0f / x, ry = 1.0f / y, rz = 1.0f / z;
}
}  // namespace ieee
