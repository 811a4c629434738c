// The reference's Y channel of a BGR pixel in [0, 255] (basicsr/metrics/metric_util.py to_y_channel through
// basicsr/utils/matlab_functions.py bgr2ycbcr(y_only=True)), shared by niqe.hip and psnr_ssim.hip:
// v = fl32(x / 255); d = b 24.966 + g 128.553 + r 65.481 + 16 in float64; Y = fl32(fl32(d / 255) * 255).
#pragma once
#include <hip/hip_runtime.h>

// numpy's arithmetic: a product and a sum are two roundings.  No contraction to FMA.
#pragma clang fp contract(off)

namespace nbp {

__device__ __forceinline__ float luma_of(float b, float g, float r) {
  const float vb = b / 255.0f, vg = g / 255.0f, vr = r / 255.0f;
  const double d = (((double)vb * 24.966 + (double)vg * 128.553) + (double)vr * 65.481) + 16.0;
  const float y = (float)(d / 255.0);
  return y * 255.0f;
}

// an image that is not three-channel: to_y_channel only scales it down and up again, in float32
__device__ __forceinline__ float luma_of(float x) { return (x / 255.0f) * 255.0f; }

}  // namespace nbp
