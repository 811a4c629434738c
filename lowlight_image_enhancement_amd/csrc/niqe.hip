// NIQE, the reference's no-reference quality metric (NAFNet_base/basicsr/metrics/niqe.py, calculate_niqe with
// convert_to='y'), on the caller's stream without a host synchronisation:
//   * nbp_niqe_luma: strided uint8 / float32 BGR pixels (any of HWC, CHW, HW through a row, a pixel and a channel
//     stride) -> the float32 Y plane, cut to whole 96 x 96 blocks.
//   * nbp_niqe_features: the half-size plane of scale 2 (2 x 2 pair means), then one work-group per (scale, block):
//     the block's Y tile with its 3-pixel halo goes through LDS in two strips, the MSCN block is written to LDS and
//     never to memory, the moments of the block and of its four circular pair products are reduced in a fixed order,
//     five table searches give the AGGD shapes and the group writes its 18 features.
//   * nbp_niqe_score: one work-group: column nanmeans, the covariance of the NaN-free rows, a float64 Cholesky solve
//     of (cov_pris + cov) / 2 against mu_pris - mu, and the root of the quadratic form.
// Where the reference rounds to float32 (scipy.ndimage.convolve returns its input's type) the kernels round too; the
// window sums, the moments and everything after them are float64.  Over a constant region the float64 window sum
// makes mu == x and sigma == 0 exactly, so the normalised map is exactly 0 there, which the reference's NaN handling
// (empty x < 0 and x > 0 sets) depends on.  No floating-point atomics: every reduction is fixed-order, so results are
// reproducible run to run.
#include <math.h>

#include "luma.h"
#include "nbp_common.h"

using namespace nbp;

// The reference's arithmetic is numpy's and scipy's: a product and a sum are two roundings.  No contraction to FMA.
#pragma clang fp contract(off)

namespace {

constexpr int NQ_BLOCK = 96;      // block edge at scale 1 (48 at scale 2)
constexpr int NQ_HALO = 3;        // the 7 x 7 window
constexpr int NQ_TABLE = 9801;    // gam = 0.2 ... 10.000 in steps of 0.001
constexpr int NQ_THREADS = 512;
constexpr int NQ_WAVES = NQ_THREADS / 64;
constexpr int NQ_MOM = 5;         // per map: count(x<0), sum x^2 (x<0), count(x>0), sum x^2 (x>0), sum |x|
constexpr int NQ_MAPS = 5;        // the block and its products with four circular shifts
constexpr int NQ_FEAT = 18;       // features per scale
constexpr int NQ_MAX_ROWS = 16384;  // blocks per frame the score stage keeps flags for (a 12288 x 12288 frame)

// ---------------------------------------------------------------- luma
// Three channels: luma_of (luma.h).  One channel (layout HW): the reference only casts to float32.
template <typename T>
__global__ __launch_bounds__(256) void niqe_luma_kernel(const T* __restrict__ img, int Hc, int Wc, int channels,
                                                        long row_stride, long pix_stride, long ch_stride,
                                                        float* __restrict__ y) {
  const long n = (long)Hc * Wc;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / Wc), c = (int)(i % Wc);
    const T* p = img + r * row_stride + c * pix_stride;
    y[i] = channels == 1 ? (float)p[0] : luma_of((float)p[0], (float)p[ch_stride], (float)p[2 * ch_stride]);
  }
}

// scale 2: fl32(Y / 255), the mean of horizontal pairs, then of vertical pairs (each rounded to float32), * 255
__global__ __launch_bounds__(256) void niqe_half_kernel(const float* __restrict__ y, int Hh, int Wh,
                                                        float* __restrict__ half) {
  const long n = (long)Hh * Wh;
  const long W = 2L * Wh;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / Wh), c = (int)(i % Wh);
    const float* p = y + 2L * r * W + 2L * c;
    const float a = p[0] / 255.0f, b = p[1] / 255.0f, cc = p[W] / 255.0f, d = p[W + 1] / 255.0f;
    const float top = a * 0.5f + b * 0.5f, bot = cc * 0.5f + d * 0.5f;
    half[i] = (top * 0.5f + bot * 0.5f) * 255.0f;
  }
}

// ---------------------------------------------------------------- AGGD fit
// argmin_i (r_gam[i] - r)^2 as np.argmin gives it: r_gam is strictly increasing, so the minimum lies at one of the two
// entries around r; ties go to the lower index; a NaN r (and an infinite one, whose squared distances are all equal)
// selects index 0.
__device__ int niqe_table_search(const double* __restrict__ r_gam, double r) {
  if (!(fabs(r) < INFINITY)) return 0;
  int lo = 0, hi = NQ_TABLE;  // first index with r_gam[i] >= r
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r_gam[mid] < r) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0;
  if (lo == NQ_TABLE) return NQ_TABLE - 1;
  const double a = r_gam[lo - 1] - r, b = r_gam[lo] - r;
  return (b * b < a * a) ? lo : lo - 1;
}

// ---------------------------------------------------------------- block features
// One work-group per block of one scale.  BS: block edge (96 / 48).  plane [Hp][Wp] is the Y plane of the scale, whole
// blocks in both directions; the window's border is the plane's (replicated), not the block's.
template <int BS>
__global__ __launch_bounds__(NQ_THREADS) void niqe_block_features_kernel(
    const float* __restrict__ plane, int Hp, int Wp, int nbh, const double* __restrict__ win /*[49]*/,
    const double* __restrict__ tables /*[4][NQ_TABLE]: r_gam, beta scale, mean ratio, gam*/, int col0, double* __restrict__ feat /*[blocks][36]*/) {
  constexpr int STRIP = BS / 2;                 // MSCN rows per pass over the tile
  constexpr int TW = BS + 2 * NQ_HALO;          // tile columns
  constexpr int TH = STRIP + 2 * NQ_HALO;       // tile rows
  __shared__ float tile[TH * TW];
  __shared__ float mscn[BS * BS];
  __shared__ double wl[49];
  __shared__ double red[NQ_WAVES][NQ_MAPS * NQ_MOM];
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;                   // the reference's order: idx_w outer, idx_h inner
  const int bw = blk / nbh, bh = blk % nbh;
  const int y0 = bh * BS, x0 = bw * BS;
  if (tid < 49) wl[tid] = win[tid];

  // ---- MSCN map of the block, two strips of rows
  for (int strip = 0; strip < 2; ++strip) {
    const int ys = y0 + strip * STRIP;
    __syncthreads();  // the previous strip's tile has been read
    for (int e = tid; e < TH * TW; e += NQ_THREADS) {
      int gy = ys - NQ_HALO + e / TW, gx = x0 - NQ_HALO + e % TW;
      gy = min(max(gy, 0), Hp - 1);
      gx = min(max(gx, 0), Wp - 1);
      tile[e] = plane[(long)gy * Wp + gx];
    }
    __syncthreads();
    for (int e = tid; e < STRIP * BS; e += NQ_THREADS) {
      const int ty = e / BS, tx = e % BS;
      const float* t = tile + ty * TW + tx;
      double s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int i = 0; i < 7; ++i) {  // scipy's order: the window in raster order, one float64 accumulator
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const float v = t[i * TW + j];
          const float v2 = v * v;
          const double w = wl[i * 7 + j];
          s1 = s1 + (double)v * w;
          s2 = s2 + (double)v2 * w;
        }
      }
      const float x = t[NQ_HALO * TW + NQ_HALO];
      const float mu = (float)s1;
      const float sq = (float)s2;
      const float mu2 = mu * mu;
      const float sigma = sqrtf(fabsf(sq - mu2));
      mscn[(strip * STRIP + ty) * BS + tx] = (x - mu) / (sigma + 1.0f);
    }
  }
  __syncthreads();

  // ---- moments of the five maps: b, b * b[i][j-1], b * b[i-1][j], b * b[i-1][j-1], b * b[i-1][j+1] (circular)
  double acc[NQ_MAPS * NQ_MOM];
#pragma unroll
  for (int k = 0; k < NQ_MAPS * NQ_MOM; ++k) acc[k] = 0.0;
  for (int e = tid; e < BS * BS; e += NQ_THREADS) {
    const int i = e / BS, j = e % BS;
    const int im = (i == 0 ? BS - 1 : i - 1) * BS, jm = j == 0 ? BS - 1 : j - 1, jp = j == BS - 1 ? 0 : j + 1;
    const float b = mscn[e];
    float xs[NQ_MAPS];
    xs[0] = b;
    xs[1] = b * mscn[i * BS + jm];
    xs[2] = b * mscn[im + j];
    xs[3] = b * mscn[im + jm];
    xs[4] = b * mscn[im + jp];
#pragma unroll
    for (int m = 0; m < NQ_MAPS; ++m) {
      const double x = (double)xs[m];
      const double x2 = x * x;
      if (xs[m] < 0.f) {
        acc[m * NQ_MOM + 0] += 1.0;
        acc[m * NQ_MOM + 1] += x2;
      } else if (xs[m] > 0.f) {
        acc[m * NQ_MOM + 2] += 1.0;
        acc[m * NQ_MOM + 3] += x2;
      }
      acc[m * NQ_MOM + 4] += fabs(x);
    }
  }
#pragma unroll
  for (int k = 0; k < NQ_MAPS * NQ_MOM; ++k) {
    const double v = wave_sum_d(acc[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();

  // ---- one thread per map: the fit and the map's features
  if (tid < NQ_MAPS) {
    double mom[NQ_MOM];
#pragma unroll
    for (int k = 0; k < NQ_MOM; ++k) {
      double t = 0.0;
      for (int w = 0; w < NQ_WAVES; ++w) t += red[w][tid * NQ_MOM + k];
      mom[k] = t;
    }
    const double N = (double)(BS * BS);
    const double left_std = sqrt(mom[1] / mom[0]);   // 0 / 0 = NaN: no negative sample
    const double right_std = sqrt(mom[3] / mom[2]);
    const double g = left_std / right_std;
    const double mabs = mom[4] / N;
    const double rhat = (mabs * mabs) / ((mom[1] + mom[3]) / N);
    const double g2 = g * g + 1.0;
    const double rn = (rhat * (g * g * g + 1.0) * (g + 1.0)) / (g2 * g2);
    const int idx = niqe_table_search(tables, rn);
    const double scale = tables[NQ_TABLE + idx];       // sqrt(Gamma(1/a) / Gamma(3/a))
    const double beta_l = left_std * scale, beta_r = right_std * scale;
    double* f = feat + (long)blk * (2 * NQ_FEAT) + col0;
    const double a = tables[3 * NQ_TABLE + idx];       // gam[idx]
    if (tid == 0) {
      f[0] = a;
      f[1] = (beta_l + beta_r) / 2.0;
    } else {
      double* q = f + 2 + 4 * (tid - 1);
      q[0] = a;
      q[1] = (beta_r - beta_l) * tables[2 * NQ_TABLE + idx];  // Gamma(2/a) / Gamma(1/a)
      q[2] = beta_l;
      q[3] = beta_r;
    }
  }
}

// ---------------------------------------------------------------- score
// One work-group of 1024 threads.  feat [n][36] -> out[0] = sqrt(d A^-1 d^T), d = mu_pris - nanmean(feat),
// A = (cov_pris + cov(rows of feat without NaN, ddof 1)) / 2.  Fewer than two such rows: NaN.
constexpr int SC_THREADS = 1024;
constexpr int SC_F = 2 * NQ_FEAT;             // 36
constexpr int SC_GROUPS = 14;                 // row groups per column in the mean pass (36 * 14 = 504 threads)
constexpr int SC_CHUNK = 64;                  // rows staged in LDS per covariance step

__global__ __launch_bounds__(SC_THREADS) void niqe_stats_kernel(const double* __restrict__ feat, int n,
                                                                const double* __restrict__ mu_pris,
                                                                const double* __restrict__ cov_pris,
                                                                double* __restrict__ out) {
  __shared__ unsigned char clean[NQ_MAX_ROWS];
  __shared__ double part[3][SC_GROUPS][SC_F];   // nan-free sum, its count, clean-row sum
  __shared__ double stage[SC_CHUNK][SC_F + 1];
  __shared__ double A[SC_F][SC_F + 1];
  __shared__ double mean_all[SC_F], mean_clean[SC_F], dvec[SC_F];
  __shared__ double n_clean_s;
  const int tid = threadIdx.x;
  for (int r = tid; r < n; r += SC_THREADS) {
    bool ok = true;
    for (int c = 0; c < SC_F; ++c) {
      const double v = feat[(long)r * SC_F + c];
      ok = ok && !(v != v);
    }
    clean[r] = ok ? 1 : 0;
  }
  __syncthreads();
  // column sums: thread (g, c) takes rows g, g + SC_GROUPS, ... in order
  if (tid < SC_GROUPS * SC_F) {
    const int g = tid / SC_F, c = tid % SC_F;
    double s = 0.0, cnt = 0.0, sc = 0.0;
    for (int r = g; r < n; r += SC_GROUPS) {
      const double v = feat[(long)r * SC_F + c];
      if (!(v != v)) {
        s += v;
        cnt += 1.0;
      }
      if (clean[r]) sc += v;
    }
    part[0][g][c] = s;
    part[1][g][c] = cnt;
    part[2][g][c] = sc;
  }
  __syncthreads();
  if (tid < SC_F) {
    double s = 0.0, cnt = 0.0, sc = 0.0;
    for (int g = 0; g < SC_GROUPS; ++g) {
      s += part[0][g][tid];
      cnt += part[1][g][tid];
      sc += part[2][g][tid];
    }
    double nc = 0.0;
    for (int r = 0; r < n; ++r) nc += clean[r] ? 1.0 : 0.0;
    mean_all[tid] = s / cnt;      // a column of NaNs alone: 0 / 0 = NaN, as np.nanmean
    mean_clean[tid] = sc / nc;
    if (tid == 0) n_clean_s = nc;
  }
  __syncthreads();
  // covariance of the clean rows: centred rows staged in LDS (zero rows for the others), each thread one or two entries
  double c0 = 0.0, c1 = 0.0;
  const int e0 = tid, e1 = tid + SC_THREADS;  // entries (i, j) = (e / 36, e % 36) of the 1296
  for (int base = 0; base < n; base += SC_CHUNK) {
    __syncthreads();
    for (int e = tid; e < SC_CHUNK * SC_F; e += SC_THREADS) {
      const int r = base + e / SC_F, c = e % SC_F;
      stage[e / SC_F][c] = (r < n && clean[r]) ? feat[(long)r * SC_F + c] - mean_clean[c] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < SC_CHUNK; ++r) {
      c0 += stage[r][e0 / SC_F] * stage[r][e0 % SC_F];
      if (e1 < SC_F * SC_F) c1 += stage[r][e1 / SC_F] * stage[r][e1 % SC_F];
    }
  }
  const double denom = n_clean_s - 1.0;  // one clean row: 0 / 0 = NaN; none: the means are NaN already
  A[e0 / SC_F][e0 % SC_F] = (cov_pris[e0] + c0 / denom) / 2.0;
  if (e1 < SC_F * SC_F) A[e1 / SC_F][e1 % SC_F] = (cov_pris[e1] + c1 / denom) / 2.0;
  if (tid < SC_F) dvec[tid] = mu_pris[tid] - mean_all[tid];
  __syncthreads();
  // Cholesky A = L L^T in place (lower triangle), then L y = d and q = sqrt(y . y)
  for (int k = 0; k < SC_F; ++k) {
    if (tid == 0) A[k][k] = sqrt(A[k][k]);  // not positive definite (or NaN): NaN from here on
    __syncthreads();
    if (tid > k && tid < SC_F) A[tid][k] = A[tid][k] / A[k][k];
    __syncthreads();
    if (tid > k && tid < SC_F) {
      const double lik = A[tid][k];
      for (int j = k + 1; j <= tid; ++j) A[tid][j] -= lik * A[j][k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double q = 0.0;
    for (int i = 0; i < SC_F; ++i) {
      double s = dvec[i];
      for (int j = 0; j < i; ++j) s -= A[i][j] * dvec[j];
      s = s / A[i][i];
      dvec[i] = s;
      q += s * s;
    }
    out[0] = sqrt(q);
  }
}

inline int stream_blocks(long n) {
  long b = (n + 1023) / 1024;  // >= 4 elements per thread
  if (b > 2048) b = 2048;
  return (int)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

size_t nbp_niqe_workspace_bytes(int H, int W) {
  if (H < NQ_BLOCK || W < NQ_BLOCK) return 0;
  const size_t hh = (size_t)(H / NQ_BLOCK) * (NQ_BLOCK / 2), wh = (size_t)(W / NQ_BLOCK) * (NQ_BLOCK / 2);
  return hh * wh * sizeof(float);
}

int nbp_niqe_luma(const void* img, int is_u8, int H, int W, int channels, long row_stride, long pix_stride,
                  long ch_stride, float* y, nbp_stream_t s) {
  NBP_REQUIRE(img && y, "nbp_niqe_luma: null pointer");
  NBP_REQUIRE(H >= NQ_BLOCK && W >= NQ_BLOCK, "nbp_niqe_luma: the frame %d x %d holds no 96 x 96 block", H, W);
  NBP_REQUIRE(channels == 1 || channels == 3, "nbp_niqe_luma: 1 or 3 channels, got %d", channels);
  const int Hc = H / NQ_BLOCK * NQ_BLOCK, Wc = W / NQ_BLOCK * NQ_BLOCK;
  const int g = stream_blocks((long)Hc * Wc);
  if (is_u8)
    niqe_luma_kernel<unsigned char><<<g, 256, 0, S(s)>>>(static_cast<const unsigned char*>(img), Hc, Wc, channels,
                                                         row_stride, pix_stride, ch_stride, y);
  else
    niqe_luma_kernel<float><<<g, 256, 0, S(s)>>>(static_cast<const float*>(img), Hc, Wc, channels, row_stride,
                                                 pix_stride, ch_stride, y);
  return check_launch("niqe_luma");
}

int nbp_niqe_features(const float* y, int H, int W, const double* window, const double* tables, void* ws, double* feat,
                      nbp_stream_t s) {
  NBP_REQUIRE(y && window && tables && ws && feat, "nbp_niqe_features: null pointer");
  NBP_REQUIRE(H >= NQ_BLOCK && W >= NQ_BLOCK, "nbp_niqe_features: the frame %d x %d holds no 96 x 96 block", H, W);
  const int nbh = H / NQ_BLOCK, nbw = W / NQ_BLOCK;
  const int Hc = nbh * NQ_BLOCK, Wc = nbw * NQ_BLOCK;
  float* half = static_cast<float*>(ws);
  niqe_half_kernel<<<stream_blocks((long)(Hc / 2) * (Wc / 2)), 256, 0, S(s)>>>(y, Hc / 2, Wc / 2, half);
  niqe_block_features_kernel<NQ_BLOCK><<<nbh * nbw, NQ_THREADS, 0, S(s)>>>(y, Hc, Wc, nbh, window, tables, 0, feat);
  niqe_block_features_kernel<NQ_BLOCK / 2><<<nbh * nbw, NQ_THREADS, 0, S(s)>>>(half, Hc / 2, Wc / 2, nbh, window, tables,
                                                                              NQ_FEAT, feat);
  return check_launch("niqe_features");
}

int nbp_niqe_score(const double* feat, int rows, const double* mu_pris, const double* cov_pris, double* out,
                   nbp_stream_t s) {
  NBP_REQUIRE(feat && mu_pris && cov_pris && out, "nbp_niqe_score: null pointer");
  NBP_REQUIRE(rows >= 1 && rows <= NQ_MAX_ROWS, "nbp_niqe_score: rows must be in [1, %d], got %d", NQ_MAX_ROWS, rows);
  niqe_stats_kernel<<<1, SC_THREADS, 0, S(s)>>>(feat, rows, mu_pris, cov_pris, out);
  return check_launch("niqe_score");
}

}  // extern "C"
