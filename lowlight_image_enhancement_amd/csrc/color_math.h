// Per-pixel colour arithmetic shared by color.hip and valstats.hip (both compile this text): fp32 values or dual
// numbers carrying d/d(R,G,B), kornia-0.6.12 rgb_to_lab, the metric-form CIEDE2000 and clamp01.
#pragma once
#include "nbp_common.h"

namespace {

struct D3 {
  float v, d0, d1, d2;
};
__device__ __forceinline__ D3 mk(float v) { return D3{v, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ D3 scl(const D3& a, float dv, float vv) { return D3{vv, a.d0 * dv, a.d1 * dv, a.d2 * dv}; }
__device__ __forceinline__ D3 operator+(const D3& a, const D3& b) { return D3{a.v + b.v, a.d0 + b.d0, a.d1 + b.d1, a.d2 + b.d2}; }
__device__ __forceinline__ D3 operator-(const D3& a, const D3& b) { return D3{a.v - b.v, a.d0 - b.d0, a.d1 - b.d1, a.d2 - b.d2}; }
__device__ __forceinline__ D3 operator*(const D3& a, const D3& b) {
  return D3{a.v * b.v, a.d0 * b.v + a.v * b.d0, a.d1 * b.v + a.v * b.d1, a.d2 * b.v + a.v * b.d2};
}
__device__ __forceinline__ D3 operator/(const D3& a, const D3& b) {
  const float q = a.v / b.v, ib = 1.f / b.v;
  return D3{q, (a.d0 - q * b.d0) * ib, (a.d1 - q * b.d1) * ib, (a.d2 - q * b.d2) * ib};
}
__device__ __forceinline__ D3 operator+(const D3& a, float b) { return D3{a.v + b, a.d0, a.d1, a.d2}; }
__device__ __forceinline__ D3 operator+(float b, const D3& a) { return a + b; }
__device__ __forceinline__ D3 operator-(const D3& a, float b) { return D3{a.v - b, a.d0, a.d1, a.d2}; }
__device__ __forceinline__ D3 operator-(float b, const D3& a) { return D3{b - a.v, -a.d0, -a.d1, -a.d2}; }
__device__ __forceinline__ D3 operator-(const D3& a) { return D3{-a.v, -a.d0, -a.d1, -a.d2}; }
__device__ __forceinline__ D3 operator*(const D3& a, float b) { return D3{a.v * b, a.d0 * b, a.d1 * b, a.d2 * b}; }
__device__ __forceinline__ D3 operator*(float b, const D3& a) { return a * b; }
__device__ __forceinline__ D3 operator/(const D3& a, float b) { return D3{a.v / b, a.d0 / b, a.d1 / b, a.d2 / b}; }

__device__ __forceinline__ float val(float x) { return x; }
__device__ __forceinline__ float val(const D3& x) { return x.v; }

__device__ __forceinline__ float vsqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ D3 vsqrt(const D3& x) {
  const float r = sqrtf(x.v);
  return scl(x, 0.5f / r, r);
}
__device__ __forceinline__ float vpow(float x, float c) { return powf(x, c); }
__device__ __forceinline__ D3 vpow(const D3& x, float c) { return scl(x, c * powf(x.v, c - 1.f), powf(x.v, c)); }
__device__ __forceinline__ float vsin(float x) { return sinf(x); }
__device__ __forceinline__ D3 vsin(const D3& x) { return scl(x, cosf(x.v), sinf(x.v)); }
__device__ __forceinline__ float vcos(float x) { return cosf(x); }
__device__ __forceinline__ D3 vcos(const D3& x) { return scl(x, -sinf(x.v), cosf(x.v)); }
__device__ __forceinline__ float vexp(float x) { return expf(x); }
__device__ __forceinline__ D3 vexp(const D3& x) {
  const float e = expf(x.v);
  return scl(x, e, e);
}
__device__ __forceinline__ float vatan2(float y, float x) { return atan2f(y, x); }
// torch's atan2 backward is defined as 0 at the origin (a grey pixel: a' = b = 0)
__device__ __forceinline__ D3 vatan2(const D3& y, const D3& x) {
  const float den = x.v * x.v + y.v * y.v, v = atan2f(y.v, x.v);
  if (den == 0.f) return mk(v);
  return D3{v, (x.v * y.d0 - y.v * x.d0) / den, (x.v * y.d1 - y.v * x.d1) / den, (x.v * y.d2 - y.v * x.d2) / den};
}
// torch remainder (sign of the divisor): a - b * floor(a / b); d/da = 1
__device__ __forceinline__ float vmod(float a, float b) { return a - b * floorf(a / b); }
__device__ __forceinline__ D3 vmod(const D3& a, float b) { return D3{vmod(a.v, b), a.d0, a.d1, a.d2}; }
// clamp(min=lo): identity slope where x >= lo (torch's inclusive mask), constant below
__device__ __forceinline__ float vclamp_min(float x, float lo) { return fmaxf(x, lo); }
__device__ __forceinline__ D3 vclamp_min(const D3& x, float lo) { return x.v >= lo ? x : mk(lo); }
template <typename V>
__device__ __forceinline__ V sel(bool c, const V& a, const V& b) { return c ? a : b; }

constexpr float PI_F = 3.14159265358979323846f;
constexpr float TWO_PI_F = 6.28318530717958647692f;
constexpr float P25 = 6103515625.f;  // 25**7 as the fp32 scalar torch adds
constexpr float DEG2RAD = 0.017453292519943295f, RAD2DEG = 57.29577951308232f;

// kornia 0.6.12 color.rgb_to_lab for one pixel (inputs already clamped as the caller requires)
template <typename V>
__device__ __forceinline__ void rgb_to_lab(const V& r0, const V& g0, const V& b0, V& L, V& A, V& Bc) {
  auto lin = [](const V& x) { return sel(val(x) > 0.04045f, vpow((x + 0.055f) / 1.055f, 2.4f), x / 12.92f); };
  const V r = lin(r0), g = lin(g0), b = lin(b0);
  const V X = 0.412453f * r + 0.357580f * g + 0.180423f * b;
  const V Y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
  const V Z = 0.019334f * r + 0.119193f * g + 0.950227f * b;
  auto f = [](const V& t) {
    const float thr = 0.008856f;
    return sel(val(t) > thr, vpow(vclamp_min(t, thr), 1.f / 3.f), 7.787f * t + 4.f / 29.f);
  };
  const V fx = f(X / 0.95047f), fy = f(Y / 1.f), fz = f(Z / 1.08883f);
  L = 116.f * fy - 16.f;
  A = 500.f * (fx - fy);
  Bc = 200.f * (fy - fz);
}

// _deltaE00_lab_map (color_error.py:105-210), per pixel (no gradient: a no-grad metric)
__device__ __forceinline__ float ciede2000_metric(float L1, float a1, float b1, float L2, float a2, float b2, float kL,
                                                  float kC, float kH, float eps) {
  const float c1 = sqrtf(a1 * a1 + b1 * b1 + eps), c2 = sqrtf(a2 * a2 + b2 * b2 + eps);
  const float cb7 = powf(0.5f * (c1 + c2), 7.f);
  const float g = 0.5f * (1.f - sqrtf(cb7 / (cb7 + P25 + eps)));
  const float a1p = (1.f + g) * a1, a2p = (1.f + g) * a2;
  const float c1p = sqrtf(a1p * a1p + b1 * b1 + eps), c2p = sqrtf(a2p * a2p + b2 * b2 + eps);
  const float h1p = atan2f(b1, a1p), h2p = atan2f(b2, a2p);
  const float dLp = L2 - L1, dCp = c2p - c1p;
  const bool valid = (c1p * c2p) != 0.f;
  const float diff = h2p - h1p;
  float dh = 0.f;
  if (valid) {
    if (fabsf(diff) <= PI_F) dh = diff;
    else if (diff > PI_F) dh = diff - 2.f * PI_F;
    else dh = diff + 2.f * PI_F;
  }
  const float dHp = 2.f * sqrtf(c1p * c2p + eps) * sinf(dh / 2.f);
  const float Lbp = 0.5f * (L1 + L2), Cbp = 0.5f * (c1p + c2p);
  const float hs = h1p + h2p, ad = fabsf(h1p - h2p);
  const float hb = !valid ? hs : (ad <= PI_F ? 0.5f * hs : (hs < 2.f * PI_F ? 0.5f * (hs + 2.f * PI_F) : 0.5f * (hs - 2.f * PI_F)));
  const float r30 = 30.f * PI_F / 180.f, r6 = 6.f * PI_F / 180.f, r63 = 63.f * PI_F / 180.f;
  const float T = 1.f - 0.17f * cosf(hb - r30) + 0.24f * cosf(2.f * hb) + 0.32f * cosf(3.f * hb + r6) -
                  0.20f * cosf(4.f * hb - r63);
  const float u = ((hb * 180.f / PI_F) - 275.f) / 25.f;
  const float dtheta = r30 * expf(-(u * u));
  const float cbp7 = powf(Cbp, 7.f);
  const float RC = 2.f * sqrtf(cbp7 / (cbp7 + P25 + eps));
  const float RT = -sinf(2.f * dtheta) * RC;
  const float l50 = Lbp - 50.f;
  const float SL = 1.f + (0.015f * l50 * l50) / sqrtf(20.f + l50 * l50 + eps);
  const float SC = 1.f + 0.045f * Cbp, SH = 1.f + 0.015f * Cbp * T;
  const float tL = dLp / (kL * SL + eps), tC = dCp / (kC * SC + eps), tH = dHp / (kH * SH + eps);
  return sqrtf(fmaxf(tL * tL + tC * tC + tH * tH + RT * tC * tH, 0.f));
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

}  // namespace
