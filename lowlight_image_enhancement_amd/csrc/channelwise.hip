// Channel-wise RGB PSNR / CPSNR on device (reference: metrics/channelwise.py:111-222, rgb_psnr and cpsnr_rgb).
//   * one pass over pred and tgt [N][3][L] fp32: per plane sse = sum (double(clamp(p)) - double(clamp(t)))^2, the
//     difference taken after widening as the reference's pred.to(float64) does, the clamp to [0, clamp_hi] in float64;
//   * a plane is cut into chunks of whole 4-element groups; a block owns one (plane, chunk), thread t takes the groups
//     t, t + 256, ... of its chunk and the block sum is the fixed-order block_sum_d: the element -> thread assignment and
//     the order of every addition depend on (N, L) alone.  A chunk whose two base addresses are 16-byte aligned loads
//     its full groups as float4, any other chunk (a plane of odd length leaves the next one misaligned) and the last
//     partial group load scalars -- the same values in the same order;
//   * the finish launch (one block per image) adds a plane's chunk partials in ascending chunk order and forms
//     mse = sse / L, the three PSNRs 10 log10(range^2 / max(mse, eps)), their mean and CPSNR from the mean of the MSEs.
// No atomics: the same bits on every run.  Element offsets are 64-bit.
#include <math.h>

#include "nbp_common.h"

using namespace nbp;

namespace {

__device__ __forceinline__ double sq_diff(float p, float t, int clamp, double hi) {
  double a = (double)p, b = (double)t;
  if (clamp) {
    a = fmin(fmax(a, 0.0), hi);
    b = fmin(fmax(b, 0.0), hi);
  }
  const double d = a - b;
  return d * d;
}

__global__ __launch_bounds__(256) void rgb_sqerr_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                        long L, long per, int chunks, int clamp, double hi,
                                                        double* __restrict__ slab) {
  __shared__ double red[16];
  const long plane = blockIdx.y;
  const long l0 = (long)blockIdx.x * per, l1 = min(L, l0 + per);  // per is a multiple of 4
  double acc = 0.0;
  if (l0 < l1) {
    const float* pa = pred + plane * L + l0;
    const float* pb = tgt + plane * L + l0;
    const long len = l1 - l0, full = len / 4;
    const bool vec = ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 15) == 0;
    if (vec) {
      for (long g = threadIdx.x; g < full; g += 256) {
        const float4 a = ld4(pa + 4 * g), b = ld4(pb + 4 * g);
        acc += sq_diff(a.x, b.x, clamp, hi);
        acc += sq_diff(a.y, b.y, clamp, hi);
        acc += sq_diff(a.z, b.z, clamp, hi);
        acc += sq_diff(a.w, b.w, clamp, hi);
      }
    } else {
      for (long g = threadIdx.x; g < full; g += 256) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += sq_diff(pa[4 * g + e], pb[4 * g + e], clamp, hi);
      }
    }
    if ((long)threadIdx.x == full % 256)  // the partial last group, on the thread whose turn it is
      for (long i = 4 * full; i < len; ++i) acc += sq_diff(pa[i], pb[i], clamp, hi);
  }
  const double t = block_sum_d(acc, red);
  if (threadIdx.x == 0) slab[plane * chunks + blockIdx.x] = t;
}

// one block per image: the image's 3 * chunks partials are staged in LDS by the whole block (a single thread walking
// them in HBM pays a memory latency per handful of loads), then one thread per plane adds its row in ascending order
constexpr int kMaxChunks = 1024;

__global__ __launch_bounds__(256) void rgb_psnr_finish(const double* __restrict__ slab, int chunks, long L,
                                                       double range_sq, double eps, double* __restrict__ out) {
  __shared__ double part[3 * kMaxChunks];
  __shared__ double mse[3];
  const long n = blockIdx.x;
  for (int i = threadIdx.x; i < 3 * chunks; i += blockDim.x) part[i] = slab[n * 3 * chunks + i];
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* row = part + threadIdx.x * chunks;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += row[k];
    mse[threadIdx.x] = s / (double)L;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double psnr[3];
  for (int c = 0; c < 3; ++c) psnr[c] = 10.0 * log10(range_sq / fmax(mse[c], eps));
  double* o = out + n * 5;
  o[0] = psnr[0];
  o[1] = psnr[1];
  o[2] = psnr[2];
  o[3] = (psnr[0] + psnr[1] + psnr[2]) / 3.0;
  const double cmse = (mse[0] + mse[1] + mse[2]) / 3.0;
  o[4] = 10.0 * log10(range_sq / fmax(cmse, eps));
}

// chunks per plane: >= 4096 elements per block, about 2048 blocks in all, at most 1024 per plane
inline int rgb_chunks(long L, long planes) {
  long c = (L + 4095) / 4096;
  const long want = (2048 + planes - 1) / planes;
  if (c > want) c = want;
  if (c < 1) c = 1;
  if (c > kMaxChunks) c = kMaxChunks;
  return (int)c;
}

}  // namespace

extern "C" {

size_t nbp_rgb_psnr_workspace_doubles(int N, long L) {
  if (N <= 0 || L <= 0) return 0;
  return (size_t)N * 3 * rgb_chunks(L, (long)N * 3);
}

int nbp_rgb_psnr(const float* pred, const float* tgt, int N, long L, double data_range, double eps, int clamp,
                 double clamp_hi, double* ws, double* out, nbp_stream_t s) {
  NBP_REQUIRE(pred && tgt && ws && out && N > 0 && L > 0 && (long)N * 3 <= 65535, "nbp_rgb_psnr: bad args");
  NBP_REQUIRE(data_range > 0.0 && eps > 0.0, "nbp_rgb_psnr: data_range and eps must be positive");
  const int chunks = rgb_chunks(L, (long)N * 3);
  const long per = ((L + chunks - 1) / chunks + 3) / 4 * 4;
  rgb_sqerr_kernel<<<dim3(chunks, N * 3), 256, 0, S(s)>>>(pred, tgt, L, per, chunks, clamp ? 1 : 0, clamp_hi, ws);
  rgb_psnr_finish<<<N, 256, 0, S(s)>>>(ws, chunks, L, data_range * data_range, eps, out);
  return check_launch("rgb_psnr");
}

}  // extern "C"
