// lgamma differences for the Negative-Binomial terms, without libm's lgamma: shared by the rate update of the sampler
// (nb_loglik_kernel, btf_kernels.h) and the Negative-Binomial criteria (btf_nb_criteria.h).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace btf {

constexpr int NB_FAST_MAX = 32;    // integer counts up to here: product form when R varies inside a block
constexpr int NB_TAB = 1024;       // integer counts below this: LDS table when R is constant inside a block

// lgamma(x) for x >= NB_STIRLING_MIN by Stirling's series (truncation error < 1/(1188 x^9) = 4e-17 at x = 33)
constexpr double NB_STIRLING_MIN = 33.0;
__device__ __forceinline__ double lgamma_big(double x) {
  const double ix = 1.0 / x, ix2 = ix * ix;
  const double ser = ix * (8.3333333333333333e-2 + ix2 * (-2.7777777777777778e-3 + ix2 * (7.9365079365079365e-4 + ix2 * -5.9523809523809524e-4)));
  return (x - 0.5) * log(x) - x + 0.91893853320467274178 + ser;
}

// lgamma(a) - lgamma(b) for a, b > 0 without libm's lgamma (which costs ~200 registers): both arguments
// are shifted up by the same n until Stirling applies,
//   lgamma(a) - lgamma(b) = lgamma_big(a+n) - lgamma_big(b+n) - log( prod_{k<n}(a+k) / prod_{k<n}(b+k) ).
__device__ inline double lgamma_diff(double a, double b) {
  const double lo = fmin(a, b);
  if (lo >= NB_STIRLING_MIN) return lgamma_big(a) - lgamma_big(b);
  const int n = (int)ceil(NB_STIRLING_MIN - lo);                                   // <= 33
  double pa = 1.0, pb = 1.0;
  for (int k = 0; k < n; ++k) { pa *= a + k; pb *= b + k; }                        // < 66^33: no overflow
  return lgamma_big(a + n) - lgamma_big(b + n) - log(pa / pb);
}

// count part of one replicate's term: lgamma(y+c) - lgamma(c) - lgamma(y+r) + lgamma(r);
// base = lgamma(r) - lgamma(c) (NaN: not computed yet - filled on first use)
__device__ inline double nb_count_part(double y, double r, double c, double& base) {
  if (y >= 0.0 && y <= (double)NB_FAST_MAX && y == floor(y)) {   // = log prod_{k<y} (c+k)/(r+k)
    double num = 1.0, den = 1.0;
    const int n = (int)y;
    for (int k = 0; k < n; ++k) { num *= c + k; den *= r + k; }
    return log(num / den);
  }
  if (!(base == base)) base = lgamma_diff(r, c);
  return lgamma_diff(y + c, y + r) + base;
}

// lgamma(y + r) - lgamma(r) for y >= 0, r > 0: the sample-dependent part of a Negative-Binomial observation's constant.
// Integer y <= NB_FAST_MAX: log prod_{k<y} (r+k), nb_count_part's product form with the other rate's factors left out
// (r < NB_RISE_RMAX keeps the product of 32 factors finite); everything else by Stirling on both arguments, the smaller
// one (r) shifted up to NB_STIRLING_MIN first when it lies below - lgamma_diff with each argument shifted only as far as
// it needs, so that a count of any size leaves its product finite.
constexpr double NB_RISE_RMAX = 1e9;
__device__ inline double nb_lgamma_rise(double y, double r) {
  if (y <= (double)NB_FAST_MAX && y == floor(y) && r < NB_RISE_RMAX) {
    double p = 1.0;
    const int n = (int)y;
    for (int k = 0; k < n; ++k) p *= r + k;
    return log(p);
  }
  const double a = y + r;
  if (a < NB_STIRLING_MIN) return lgamma_diff(a, r);              // both small: the common shift (a non-integer y < 32)
  if (r >= NB_STIRLING_MIN) {
    // lgamma_big(a) - lgamma_big(r) with the two (x - 1/2) log x - x terms taken together,
    //   (r - 1/2) log1p(y / r) + y log(a) - y,
    // so that a rate far above the count (the Poisson limit) does not cancel two numbers of size r log r
    const double ia = 1.0 / a, ia2 = ia * ia, ir = 1.0 / r, ir2 = ir * ir;
    const double sa = ia * (8.3333333333333333e-2 + ia2 * (-2.7777777777777778e-3 + ia2 * (7.9365079365079365e-4 + ia2 * -5.9523809523809524e-4)));
    const double sr = ir * (8.3333333333333333e-2 + ir2 * (-2.7777777777777778e-3 + ir2 * (7.9365079365079365e-4 + ir2 * -5.9523809523809524e-4)));
    return fma(r - 0.5, log1p(y / r), y * (log(a) - 1.0)) + (sa - sr);
  }
  const int n = (int)ceil(NB_STIRLING_MIN - r);                   // <= 33: lgamma(r) = lgamma_big(r+n) - log prod_{k<n} (r+k)
  double pb = 1.0;
  for (int k = 0; k < n; ++k) pb *= r + k;                        // < 66^33
  return lgamma_big(a) - lgamma_big(r + n) + log(pb);
}

}  // namespace btf
