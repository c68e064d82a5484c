// pt_fast_math_check.inc — device measurement of the mode's own scalar primitives against double precision (pt_selfcheck_fast_math).
// Included by pt_launch.inc inside ptk::<arith>::(anonymous), beside pt_ieee_check.inc.
// The largest error over `count` operands starting at `first` of
//   kind 0  rcp_(x)                          in ulp of the double result     x = the bit pattern first + i
//   kind 1  sqrt_(x)                         "
//   kind 2  normalize()'s 1 / sqrt(x)        "
//   kind 3  sin(2 pi u), 4  cos(2 pi u)      absolute                        u = u01 of the engine state first + i (1 .. 2^31 - 2):
//                                                                            every value a draw can return
//   kind 5  sin, 6 cos of roughness u pi / 2 absolute, roughness 1, .7, .5, .05 the specular lobe's angle as the mode forms it
//   kind 7  sin(2 pi u), 8  cos(2 pi u)      in ulp where |value| > 1e-3     the figure pt_portable_math.h states for sincos_rev
// as the mode evaluates them: fast — v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 and v_sin_f32 / v_cos_f32 on revolutions; fma — the IEEE
// sequences and ptmath::sincos_rev on revolutions; exact — the IEEE sequences and ptmath::sin_r / cos_r on the reference's
// double products.  Operands that are zero, subnormal, infinite or NaN, and results outside the normal range, are passed over
// (an ulp has no meaning there).  The maximum travels as the bit pattern of a non-negative double, which orders like an integer.
PT_DEV double ulps_of(float got, double want) {
  int e;
  (void)frexp((double)(float)want, &e);
  return fabs((double)got - want) / ldexp(1.0, e - 24);
}
// (a NaN result must not hide behind fmax)
PT_DEV double worse(double err, double e) { return e == e ? fmax(err, e) : __builtin_inf(); }
PT_DEV void mode_sincos_rev(float rev, double exact_arg, float* s, float* c) {  // exact_arg: the exact build's argument, in radians
  if (kFast) {
    *s = __builtin_amdgcn_sinf(rev), *c = __builtin_amdgcn_cosf(rev);
  } else if (kFloatTrig) {
    ptmath::sincos_rev(rev, s, c);
  } else {
    ptmath::sincos_r(exact_arg, s, c);
  }
}
__global__ void k_fast_math_check(int kind, unsigned long long first, unsigned long long count, unsigned long long* __restrict__ worst) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  const double kPi = 3.14159265358979323846;
  double err = 0.0;
  const float kRoughness[4] = {1.0f, 0.7f, 0.5f, 0.05f};
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const unsigned long long n = first + i;
    if (kind <= 2) {
      const float x = __uint_as_float((uint32_t)n);
      const float ax = __builtin_fabsf(x);
      if (!(ax >= 1.17549435e-38f && ax <= 3.40282347e+38f) || (kind != 0 && x < 0.f)) continue;
      const float got = kind == 0 ? rcp_(x) : kind == 1 ? sqrt_(x) : (kFast ? __builtin_amdgcn_rsqf(x) : ieee::rcp_sqrt(x));
      const double want = kind == 0 ? 1.0 / (double)x : kind == 1 ? sqrt((double)x) : 1.0 / sqrt((double)x);
      if (!(fabs(want) >= 1.17549435e-38 && fabs(want) <= 3.40282347e+38)) continue;
      err = worse(err, ulps_of(got, want));
    } else {
      const uint32_t xs = (uint32_t)n;
      if (xs < 1u || xs > 2147483646u) continue;
      const float u = (float)(xs - 1u) * 4.656612873077392578125e-10f;  // MinStd::u01
      if (kind == 5 || kind == 6) {
        for (int j = 0; j < 4; ++j) {
          const float rough = kRoughness[j];
          float s, c;
          // exact: float(double(roughness * u) * pi * 0.5f) handed to sincosf32 (pt_shade.inc bounce_sample)
          mode_sincos_rev(rough * u * 0.25f, (double)(float)((double)(rough * u) * kPi * (double)0.5f), &s, &c);
          const double turns = 0.25 * (double)rough * (double)u;
          err = worse(err, fabs((double)(kind == 5 ? s : c) - (kind == 5 ? sinpi(2.0 * turns) : cospi(2.0 * turns))));
        }
      } else {
        float s, c;
        mode_sincos_rev(u, (double)2.0f * kPi * (double)u, &s, &c);
        const bool is_sin = kind == 3 || kind == 7;
        const double want = is_sin ? sinpi(2.0 * (double)u) : cospi(2.0 * (double)u);
        const float got = is_sin ? s : c;
        if (kind <= 4) err = worse(err, fabs((double)got - want));
        else if (fabs(want) > 1e-3) err = worse(err, ulps_of(got, want));
      }
    }
  }
  for (int o = 32; o; o >>= 1) err = fmax(err, __shfl_xor(err, o));
  if (lane_id() == 0 && err > 0.0) atomicMax(worst, (unsigned long long)__double_as_longlong(err));
}
void launch_fast_math_check(hipStream_t s, int kind, unsigned long long first, unsigned long long count, unsigned long long* worst) {
  hipLaunchKernelGGL(k_fast_math_check, dim3(4096), dim3(kBlock), 0, s, kind, first, count, worst);
}
