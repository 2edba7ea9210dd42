#pragma clang fp contract(off)
// The inverse normal CDF and the inverse error function for prior transforms: Wichura's algorithm AS241 (PPND16, Applied
// Statistics 37 (1988) 477-484), three rational approximations of degree 7 over 7 in double precision.
//
// Self-contained: the same text is pasted into the user source of a HipCallbacks plugin (tempest_amd.trace_callbacks does it for
// torch.special.ndtri / torch.erfinv, tempest_amd.priors.DEVICE_HELPERS holds it for hand-written sources) and compiles with a
// plain host compiler.  What it computes is restated operation by operation in tempest_amd/trace.py (`_ndtri_core`): Horner forms
// from the highest coefficient down (s = s * r + c[k]), one division per region, no fused multiply-add (the pragma above; a host
// compiler that does not know it takes -ffp-contract=off).  Plain if / else: a wave skips a side that none of its lanes needs.
#ifndef TPHU_QUANTILE_H
#define TPHU_QUANTILE_H
#include <math.h>

#ifdef __HIPCC__
#define TPHU_QUANTILE_FN __host__ __device__
#else
#define TPHU_QUANTILE_FN
#endif

// c7 r^7 + ... + c1 r + c0, from the highest coefficient down
static inline TPHU_QUANTILE_FN double tphu_quantile_poly(double r, double c0, double c1, double c2, double c3, double c4, double c5,
                                                         double c6, double c7) {
#ifdef __HIP_DEVICE_COMPILE__
  // The coefficients are materialised HERE, in scalar registers (an empty statement that no instruction is emitted for).  Left to
  // itself the compiler hoists all 48 of them out of the loop the whole-step kernel calls the prior in; 96 scalar registers do not
  // exist, so they land in vector registers for the life of the kernel: 214 instead of 150 VGPRs and 2 instead of 3 waves per
  // SIMD for ten Normal columns (KERNELS.md).
  asm volatile("" : "+s"(c0), "+s"(c1), "+s"(c2), "+s"(c3), "+s"(c4), "+s"(c5), "+s"(c6), "+s"(c7));
#endif
  double s = c7;
  s = s * r + c6;
  s = s * r + c5;
  s = s * r + c4;
  s = s * r + c3;
  s = s * r + c2;
  s = s * r + c1;
  s = s * r + c0;
  return s;
}

// The standard normal quantile at p, given as q = p - 0.5 and t = min(p, 1 - p) -- the caller forms them from what it has without
// cancellation: tphu_ndtri from p, tphu_erfinv from y = 2 p - 1.  t in [0, 0.5], q of the sign of the result; t == 0: -inf / +inf.
static inline TPHU_QUANTILE_FN double tphu_ndtri_core(double q, double t) {
  if (fabs(q) <= 0.425) {                        // the central region: q A(r) / B(r)
    const double r = 0.180625 - q * q;
    const double num = tphu_quantile_poly(r, 3.3871328727963666080, 133.14166789178437745, 1971.5909503065514427,
                                          13731.693765509461125, 45921.953931549871457, 67265.770927008700853,
                                          33430.575583588128105, 2509.0809287301226727);
    const double den = tphu_quantile_poly(r, 1.0, 42.313330701600911252, 687.18700749205790830, 5394.1960214247511077,
                                          21213.794301586595867, 39307.895800092710610, 28729.085735721942674,
                                          5226.4952788528545610);
    return q * num / den;
  }
  if (!(t > 0.0))                                // p = 0 or p = 1 (a NaN never gets here: the wrappers answer it)
    return q < 0.0 ? -HUGE_VAL : HUGE_VAL;
  double r = sqrt(-log(t)), x;
  if (r <= 5.0) {                                // the near tail, t >= exp(-25): C(r - 1.6) / D(r - 1.6)
    r = r - 1.6;
    const double num = tphu_quantile_poly(r, 1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550,
                                          3.64784832476320460504, 1.27045825245236838258, 0.241780725177450611770,
                                          0.0227238449892691845833, 7.74545014278341407640e-4);
    const double den = tphu_quantile_poly(r, 1.0, 2.05319162663775882187, 1.67638483018380384940, 0.689767334985100004550,
                                          0.148103976427480074590, 0.0151986665636164571966, 5.47593808499534494600e-4,
                                          1.05075007164441684324e-9);
    x = num / den;
  } else {                                       // the far tail, down to the smallest subnormal: E(r - 5) / F(r - 5)
    r = r - 5.0;
    const double num = tphu_quantile_poly(r, 6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580,
                                          0.296560571828504891230, 0.0265321895265761230930, 0.00124266094738807843860,
                                          2.71155556874348757815e-5, 2.01033439929228813265e-7);
    const double den = tphu_quantile_poly(r, 1.0, 0.599832206555887937690, 0.136929880922735805310, 0.0148753612908506148525,
                                          7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7,
                                          2.04426310338993978564e-15);
    x = num / den;
  }
  return q < 0.0 ? -x : x;
}

// The x with Phi(x) = p: -inf at 0, +inf at 1, exactly 0 at 0.5, NaN outside [0, 1] and for a NaN (torch.special.ndtri's conventions)
static inline TPHU_QUANTILE_FN double tphu_ndtri(double p) {
  if (!(p >= 0.0 && p <= 1.0)) return NAN;
  return tphu_ndtri_core(p - 0.5, fmin(p, 1.0 - p));
}

// The x with erf(x) = y: -inf / +inf at -1 / +1, NaN outside [-1, 1] and for a NaN.  q = y / 2 keeps a tiny y's relative accuracy,
// which (y + 1) / 2 would round away (a subnormal y loses its last bit to the halving; the smallest one gives a signed zero).
static inline TPHU_QUANTILE_FN double tphu_erfinv(double y) {
  if (!(fabs(y) <= 1.0)) return NAN;
  return tphu_ndtri_core(0.5 * y, 0.5 * (1.0 - fabs(y))) * 0.70710678118654752440;
}

#endif  // TPHU_QUANTILE_H
