// The reference's image-domain PSNR and SSIM (NAFNet_base/basicsr/metrics/psnr_ssim.py: calculate_psnr, calculate_ssim
// with its three maps _ssim_3d, _ssim and _ssim_cly), on the caller's stream without a host synchronisation.  Both
// images are read in place through a row, a pixel and a channel stride (HWC, CHW, crops and channel slices need no
// copy), as uint8 or float32; no kernel reads outside the H x W x C view it is given (every index is clamped into it).
//   * nbp_bsr_psnr: one pass over both views, optionally through the Y channel (luma.h); each work-group writes the
//     float64 sum of its squared differences and whether image 1 holds a value that is not <= 1; one small group adds
//     the partials in a fixed order, picks max_value (1 or 255) and writes 20 log10(max_value / sqrt(mse)), or +inf.
//   * nbp_bsr_ssim: one work-group per 32 x 16 tile of the map.  The tile and its 5-pixel halo of both images go to
//     LDS as float32 (exact for all inputs).  Per input channel the five quantities a, b, a^2, b^2, ab are filtered with
//     the 11-tap Gaussian along the rows into LDS (float64) and along the columns into registers (float64); the 3-D map
//     then mixes the channels (the third axis of the reference's 11 x 11 x 11 kernel with its replicated border is a
//     fixed C x C matrix), the map is evaluated in float64 for max_value 1 and for 255, and the group writes both sums
//     and its "not <= 1" flag.  One small group adds the partials in a fixed order, picks the sum and divides.
// No floating-point atomics: every reduction is fixed-order, so results are reproducible run to run.
#include <math.h>

#include "luma.h"
#include "nbp_common.h"

using namespace nbp;

// The map and the Y chain are numpy's arithmetic: a product and a sum are two roundings.  No contraction to FMA; the
// Gaussian sums, whose order the reference does not define, use fma() explicitly.
#pragma clang fp contract(off)

namespace {

constexpr int BS_R = 5;                    // window radius
constexpr int BS_K = 2 * BS_R + 1;         // 11 taps
constexpr int BS_TW = 32, BS_TH = 16;      // map tile per work-group
constexpr int BS_TC = BS_TW + 2 * BS_R;    // 42 tile columns
constexpr int BS_TR = BS_TH + 2 * BS_R;    // 26 tile rows
constexpr int BS_THREADS = 256;
constexpr int BS_PPT = BS_TW * BS_TH / BS_THREADS;  // 2 map pixels per thread
constexpr int BS_PART = 3;                 // per group: map sum for max_value 1, for 255, flag
constexpr int BS_MODE_3D = 0, BS_MODE_VALID = 1, BS_MODE_Y = 2;
constexpr int PS_THREADS = 256;
constexpr int PS_MAX_BLOCKS = 1024;
constexpr int FIN_THREADS = 256;

// ---------------------------------------------------------------- PSNR
// parts[2 b] = sum over the group's pixels of (img1 - img2)^2 in float64, parts[2 b + 1] = 1 if one of its img1 values
// (Y values when Y is set) is not <= 1 (a NaN counts, as numpy's max propagates it), else 0.
template <typename T, int C, bool Y>
__global__ __launch_bounds__(PS_THREADS) void bsr_psnr_partial_kernel(const T* __restrict__ img1,
                                                                      const T* __restrict__ img2, int H, int W,
                                                                      long rs1, long ps1, long cs1, long rs2, long ps2,
                                                                      long cs2, double* __restrict__ parts) {
  __shared__ double red[16];
  const long n = (long)H * W;
  double acc = 0.0;
  int flag = 0;
  for (long i = blockIdx.x * (long)PS_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * PS_THREADS) {
    const int r = (int)(i / W), c = (int)(i % W);
    const T* p1 = img1 + r * rs1 + c * ps1;
    const T* p2 = img2 + r * rs2 + c * ps2;
    if constexpr (Y) {
      float y1, y2;
      if constexpr (C == 3) {
        y1 = luma_of((float)p1[0], (float)p1[cs1], (float)p1[2 * cs1]);
        y2 = luma_of((float)p2[0], (float)p2[cs2], (float)p2[2 * cs2]);
      } else {
        y1 = luma_of((float)p1[0]);
        y2 = luma_of((float)p2[0]);
      }
      const double d = (double)y1 - (double)y2;
      acc += d * d;
      flag |= !(y1 <= 1.0f);
    } else {
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const float a = (float)p1[k * cs1], b = (float)p2[k * cs2];
        const double d = (double)a - (double)b;
        acc += d * d;
        flag |= !(a <= 1.0f);
      }
    }
  }
  const double s = block_sum_d(acc, red);
  const int any = __syncthreads_or(flag);
  if (threadIdx.x == 0) {
    parts[2 * blockIdx.x] = s;
    parts[2 * blockIdx.x + 1] = any ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(FIN_THREADS) void bsr_psnr_final_kernel(const double* __restrict__ parts, int nparts,
                                                                     double count, double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0, f = 0.0;
  for (int i = threadIdx.x; i < nparts; i += FIN_THREADS) {
    s += parts[2 * i];
    f += parts[2 * i + 1];
  }
  s = block_sum_d(s, red);
  f = block_sum_d(f, red);
  if (threadIdx.x == 0) {
    const double mse = s / count;
    const double max_value = f > 0.0 ? 255.0 : 1.0;
    out[0] = mse == 0.0 ? (double)INFINITY : 20.0 * log10(max_value / sqrt(mse));
  }
}

// ---------------------------------------------------------------- SSIM
// the map value of one pixel from its five filtered quantities, as the reference writes it
__device__ __forceinline__ double ssim_value(double mu1, double mu2, double e11, double e22, double e12, double c1,
                                             double c2) {
  const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const double sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
  return ((2.0 * mu1_mu2 + c1) * (2.0 * sigma12 + c2)) / ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2));
}

// CIN: channels of the views (1 or 3).  MODE 3-D: the map is Ho x Wo x CIN = H x W x CIN, replicated border on all
// three axes, a^2, b^2, ab rounded to float32.  MODE valid: Ho x Wo = (H - 10) x (W - 10) per channel, float64
// products.  MODE Y: the Y plane of both views (luma.h), H x W, replicated border, float64 products.
template <typename T, int CIN, int MODE>
__global__ __launch_bounds__(BS_THREADS) void bsr_ssim_tile_kernel(const T* __restrict__ img1,
                                                                   const T* __restrict__ img2, int H, int W, long rs1,
                                                                   long ps1, long cs1, long rs2, long ps2, long cs2,
                                                                   const double* __restrict__ g /*[11]*/, int Ho,
                                                                   int Wo, int tiles_x, double* __restrict__ parts) {
  constexpr int CP = MODE == BS_MODE_Y ? 1 : CIN;  // planes that are filtered
  __shared__ float ta[CP][BS_TR][BS_TC];
  __shared__ float tb[CP][BS_TR][BS_TC];
  __shared__ double hq[5][BS_TR][BS_TW];
  __shared__ double gs[BS_K];
  __shared__ double mix[CP][CP];
  __shared__ double red[16];
  const int tid = threadIdx.x;
  const int tx0 = (blockIdx.x % tiles_x) * BS_TW, ty0 = (blockIdx.x / tiles_x) * BS_TH;
  // input coordinate of tile element (0, 0): the valid map's pixel (y, x) covers input rows y ... y + 10
  const int iy0 = MODE == BS_MODE_VALID ? ty0 : ty0 - BS_R, ix0 = MODE == BS_MODE_VALID ? tx0 : tx0 - BS_R;

  if (tid < BS_K) gs[tid] = g[tid];
  if (tid < CP * CP) {  // output channel c, tap d reads channel clamp(c + d - 5): the weight each channel collects
    const int c = tid / CP, ch = tid % CP;
    double s = 0.0;
    for (int d = 0; d < BS_K; ++d)
      if (min(max(c + d - BS_R, 0), CP - 1) == ch) s += g[d];
    mix[c][ch] = s;
  }
  int flag = 0;
  for (int e = tid; e < BS_TR * BS_TC * CP; e += BS_THREADS) {
    const int ch = e % CP, pix = e / CP;
    const int r = pix / BS_TC, c = pix % BS_TC;
    const int gy = min(max(iy0 + r, 0), H - 1), gx = min(max(ix0 + c, 0), W - 1);
    const T* p1 = img1 + gy * rs1 + gx * ps1;
    const T* p2 = img2 + gy * rs2 + gx * ps2;
    float va, vb;
    if constexpr (MODE == BS_MODE_Y) {
      if constexpr (CIN == 3) {
        va = luma_of((float)p1[0], (float)p1[cs1], (float)p1[2 * cs1]);
        vb = luma_of((float)p2[0], (float)p2[cs2], (float)p2[2 * cs2]);
      } else {
        va = luma_of((float)p1[0]);
        vb = luma_of((float)p2[0]);
      }
    } else {
      va = (float)p1[ch * cs1];
      vb = (float)p2[ch * cs2];
      flag |= !(va <= 1.0f);
    }
    ta[ch][r][c] = va;
    tb[ch][r][c] = vb;
  }
  const int any = __syncthreads_or(flag);  // also the barrier behind the tile, gs and mix

  double F[BS_PPT][CP][5];
  const int px = tid % BS_TW, py = tid / BS_TW;  // this thread's map pixels: (py + 8 j, px)
#pragma unroll
  for (int ch = 0; ch < CP; ++ch) {
    // along the rows: tile row r, map column x
    for (int e = tid; e < BS_TR * BS_TW; e += BS_THREADS) {
      const int r = e / BS_TW, x = e % BS_TW;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
      for (int k = 0; k < BS_K; ++k) {
        const float a = ta[ch][r][x + k], b = tb[ch][r][x + k];
        const double w = gs[k];
        double aa, bb, ab;
        if constexpr (MODE == BS_MODE_3D) {  // the reference's float32 tensors img1 ** 2, img2 ** 2, img1 * img2
          const float faa = a * a, fbb = b * b, fab = a * b;
          aa = (double)faa;
          bb = (double)fbb;
          ab = (double)fab;
        } else {
          aa = (double)a * (double)a;
          bb = (double)b * (double)b;
          ab = (double)a * (double)b;
        }
        s0 = fma(w, (double)a, s0);
        s1 = fma(w, (double)b, s1);
        s2 = fma(w, aa, s2);
        s3 = fma(w, bb, s3);
        s4 = fma(w, ab, s4);
      }
      hq[0][r][x] = s0;
      hq[1][r][x] = s1;
      hq[2][r][x] = s2;
      hq[3][r][x] = s3;
      hq[4][r][x] = s4;
    }
    __syncthreads();
    // along the columns, into registers
#pragma unroll
    for (int j = 0; j < BS_PPT; ++j) {
      const int y = py + j * (BS_THREADS / BS_TW);
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < BS_K; ++k) s = fma(gs[k], hq[q][y + k][px], s);
        F[j][ch][q] = s;
      }
    }
    __syncthreads();  // hq is rewritten for the next channel
  }

  const double c1_1 = (0.01 * 1.0) * (0.01 * 1.0), c2_1 = (0.03 * 1.0) * (0.03 * 1.0);
  const double c1_255 = (0.01 * 255.0) * (0.01 * 255.0), c2_255 = (0.03 * 255.0) * (0.03 * 255.0);
  double acc1 = 0.0, acc255 = 0.0;
#pragma unroll
  for (int j = 0; j < BS_PPT; ++j) {
    const int oy = ty0 + py + j * (BS_THREADS / BS_TW), ox = tx0 + px;
    const bool inside = oy < Ho && ox < Wo;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      double v[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        if constexpr (MODE == BS_MODE_3D) {
          double s = 0.0;
#pragma unroll
          for (int ch = 0; ch < CP; ++ch) s = fma(mix[c][ch], F[j][ch][q], s);
          v[q] = s;
        } else {
          v[q] = F[j][c][q];
        }
      }
      if (inside) {
        acc255 += ssim_value(v[0], v[1], v[2], v[3], v[4], c1_255, c2_255);
        if constexpr (MODE != BS_MODE_Y) acc1 += ssim_value(v[0], v[1], v[2], v[3], v[4], c1_1, c2_1);
      }
    }
  }
  const double t1 = block_sum_d(acc1, red);
  const double t255 = block_sum_d(acc255, red);
  if (tid == 0) {
    parts[BS_PART * blockIdx.x] = t1;
    parts[BS_PART * blockIdx.x + 1] = t255;
    parts[BS_PART * blockIdx.x + 2] = (MODE == BS_MODE_Y || any) ? 1.0 : 0.0;
  }
}

// the mean of the map: count = Ho Wo C; an empty map (count 0) gives 0 / 0 = NaN, as numpy's mean of nothing
__global__ __launch_bounds__(FIN_THREADS) void bsr_ssim_final_kernel(const double* __restrict__ parts, int nparts,
                                                                     double count, double* __restrict__ out) {
  __shared__ double red[16];
  double s1 = 0.0, s255 = 0.0, f = 0.0;
  for (int i = threadIdx.x; i < nparts; i += FIN_THREADS) {
    s1 += parts[BS_PART * i];
    s255 += parts[BS_PART * i + 1];
    f += parts[BS_PART * i + 2];
  }
  s1 = block_sum_d(s1, red);
  s255 = block_sum_d(s255, red);
  f = block_sum_d(f, red);
  if (threadIdx.x == 0) out[0] = (f > 0.0 ? s255 : s1) / count;
}

inline int psnr_blocks(long n) {
  long b = (n + 4L * PS_THREADS - 1) / (4L * PS_THREADS);
  if (b > PS_MAX_BLOCKS) b = PS_MAX_BLOCKS;
  return (int)(b < 1 ? 1 : b);
}

struct MapDims {
  int Ho, Wo, tiles_x, tiles_y;
  long tiles;
};
inline MapDims map_dims(int H, int W, int mode) {
  MapDims d;
  d.Ho = mode == BS_MODE_VALID ? H - 2 * BS_R : H;
  d.Wo = mode == BS_MODE_VALID ? W - 2 * BS_R : W;
  if (d.Ho < 0) d.Ho = 0;
  if (d.Wo < 0) d.Wo = 0;
  d.tiles_x = (d.Wo + BS_TW - 1) / BS_TW;
  d.tiles_y = (d.Ho + BS_TH - 1) / BS_TH;
  d.tiles = (long)d.tiles_x * d.tiles_y;
  return d;
}

template <typename T>
void launch_psnr(const T* a, const T* b, int H, int W, int C, long rs1, long ps1, long cs1, long rs2, long ps2,
                 long cs2, int y, double* parts, int blocks, hipStream_t st) {
#define BSR_PSNR(CC, YY) \
  bsr_psnr_partial_kernel<T, CC, YY><<<blocks, PS_THREADS, 0, st>>>(a, b, H, W, rs1, ps1, cs1, rs2, ps2, cs2, parts)
  if (C == 3) {
    if (y) BSR_PSNR(3, true); else BSR_PSNR(3, false);
  } else {
    if (y) BSR_PSNR(1, true); else BSR_PSNR(1, false);
  }
#undef BSR_PSNR
}

template <typename T>
void launch_ssim(const T* a, const T* b, int H, int W, int C, long rs1, long ps1, long cs1, long rs2, long ps2,
                 long cs2, int mode, const double* g, const MapDims& d, double* parts, hipStream_t st) {
#define BSR_SSIM(CC, MM)                                                                                          \
  bsr_ssim_tile_kernel<T, CC, MM><<<(int)d.tiles, BS_THREADS, 0, st>>>(a, b, H, W, rs1, ps1, cs1, rs2, ps2, cs2, g, \
                                                                       d.Ho, d.Wo, d.tiles_x, parts)
  if (C == 3) {
    if (mode == BS_MODE_3D) BSR_SSIM(3, BS_MODE_3D);
    else if (mode == BS_MODE_VALID) BSR_SSIM(3, BS_MODE_VALID);
    else BSR_SSIM(3, BS_MODE_Y);
  } else {
    if (mode == BS_MODE_3D) BSR_SSIM(1, BS_MODE_3D);
    else if (mode == BS_MODE_VALID) BSR_SSIM(1, BS_MODE_VALID);
    else BSR_SSIM(1, BS_MODE_Y);
  }
#undef BSR_SSIM
}

}  // namespace

extern "C" {

size_t nbp_bsr_psnr_workspace_bytes(int H, int W) {
  if (H < 1 || W < 1) return 0;
  return (size_t)psnr_blocks((long)H * W) * 2 * sizeof(double);
}

int nbp_bsr_psnr(const void* img1, const void* img2, int is_u8, int H, int W, int C, long row_stride1,
                 long pix_stride1, long ch_stride1, long row_stride2, long pix_stride2, long ch_stride2, int y_channel,
                 void* ws, double* out, nbp_stream_t s) {
  NBP_REQUIRE(img1 && img2 && ws && out, "nbp_bsr_psnr: null pointer");
  NBP_REQUIRE(H >= 1 && W >= 1, "nbp_bsr_psnr: the view is %d x %d", H, W);
  NBP_REQUIRE(C == 1 || C == 3, "nbp_bsr_psnr: 1 or 3 channels, got %d", C);
  const int blocks = psnr_blocks((long)H * W);
  double* parts = static_cast<double*>(ws);
  if (is_u8)
    launch_psnr(static_cast<const unsigned char*>(img1), static_cast<const unsigned char*>(img2), H, W, C, row_stride1,
                pix_stride1, ch_stride1, row_stride2, pix_stride2, ch_stride2, y_channel, parts, blocks, S(s));
  else
    launch_psnr(static_cast<const float*>(img1), static_cast<const float*>(img2), H, W, C, row_stride1, pix_stride1,
                ch_stride1, row_stride2, pix_stride2, ch_stride2, y_channel, parts, blocks, S(s));
  const double count = (double)H * (double)W * (double)(y_channel ? 1 : C);
  bsr_psnr_final_kernel<<<1, FIN_THREADS, 0, S(s)>>>(parts, blocks, count, out);
  return check_launch("bsr_psnr");
}

size_t nbp_bsr_ssim_workspace_bytes(int H, int W, int mode) {
  if (H < 1 || W < 1 || mode < 0 || mode > 2) return 0;
  const MapDims d = map_dims(H, W, mode);
  return (size_t)(d.tiles < 1 ? 1 : d.tiles) * BS_PART * sizeof(double);
}

int nbp_bsr_ssim(const void* img1, const void* img2, int is_u8, int H, int W, int C, long row_stride1,
                 long pix_stride1, long ch_stride1, long row_stride2, long pix_stride2, long ch_stride2, int mode,
                 const double* window, void* ws, double* out, nbp_stream_t s) {
  NBP_REQUIRE(img1 && img2 && window && ws && out, "nbp_bsr_ssim: null pointer");
  NBP_REQUIRE(H >= 1 && W >= 1, "nbp_bsr_ssim: the view is %d x %d", H, W);
  NBP_REQUIRE(C == 1 || C == 3, "nbp_bsr_ssim: 1 or 3 channels, got %d", C);
  NBP_REQUIRE(mode >= 0 && mode <= 2, "nbp_bsr_ssim: mode 0 (3-D), 1 (valid) or 2 (Y), got %d", mode);
  const MapDims d = map_dims(H, W, mode);
  NBP_REQUIRE(d.tiles <= 0x7fffffffL, "nbp_bsr_ssim: %d x %d holds too many tiles", H, W);
  double* parts = static_cast<double*>(ws);
  if (d.tiles > 0) {
    if (is_u8)
      launch_ssim(static_cast<const unsigned char*>(img1), static_cast<const unsigned char*>(img2), H, W, C,
                  row_stride1, pix_stride1, ch_stride1, row_stride2, pix_stride2, ch_stride2, mode, window, d, parts,
                  S(s));
    else
      launch_ssim(static_cast<const float*>(img1), static_cast<const float*>(img2), H, W, C, row_stride1, pix_stride1,
                  ch_stride1, row_stride2, pix_stride2, ch_stride2, mode, window, d, parts, S(s));
  }
  const double count = (double)d.Ho * (double)d.Wo * (double)(mode == BS_MODE_Y ? 1 : C);
  bsr_ssim_final_kernel<<<1, FIN_THREADS, 0, S(s)>>>(parts, (int)d.tiles, count, out);
  return check_launch("bsr_ssim");
}

}  // extern "C"
