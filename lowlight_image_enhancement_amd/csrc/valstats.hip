// Statistics of the validation pass (validation.py, metrics/valstats.py), all on the caller's stream without a host
// synchronisation:
//   * nbp_quantile_select: two exact order statistics per row of fp32 data by radix select.  The fp32 bits are mapped to
//     order-preserving uint32 keys and the key is fixed 11 / 11 / 10 bits at a time: per pass one histogram launch
//     (LDS counts, flushed once per block into the row's global histogram) and one one-block-per-row "pick" launch that
//     scans the bins, fixes the next digits of both selectors and carries their residual ranks.  Three reads of the
//     data, no sort, no size cap below 2^31 per row.
//   * nbp_val_color_maps: one pass over pred and tgt [B][3][H][W] sRGB -> the metric-form CIEDE2000 map, |Sobel| of
//     pred's L (from an LDS tile with a one-pixel halo whose L is recomputed from pred; no Lab buffer in memory) and
//     the per-image float64 mean of the map.
//   * nbp_masked_mean: float64 sum and count of val where key >= thr[row], per row and pooled over the rows.
// Counts are unsigned-integer atomicAdd (order-independent); every floating-point reduction is fixed-order
// (per-block float64 partials, then an ordered combine), so results are reproducible run to run.
#include <math.h>

#include "color_math.h"
#include "nbp_common.h"

using namespace nbp;

namespace {

// ---------------------------------------------------------------- radix select
constexpr int QS_BINS = 2048;                                    // 11-bit digits (the last pass uses 1024 of them)
constexpr int QS_H0 = 0, QS_H1 = QS_BINS, QS_H2 = 3 * QS_BINS;   // hist0 | hist1[lo,hi] | hist2[lo,hi] (1024 each)
constexpr int QS_STATE = 4 * QS_BINS;                            // nan count, prefix lo / hi, residual rank lo / hi
constexpr int QS_WORDS = QS_STATE + 8;                           // uint32 words of workspace per row
enum { ST_NAN = 0, ST_PRE_LO = 1, ST_PRE_HI = 2, ST_RANK_LO = 3, ST_RANK_HI = 4 };

// fp32 bits -> uint32 whose unsigned order is the order of the floats (-0.0 just below +0.0, NaNs at the two ends)
__device__ __forceinline__ unsigned key_of(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// PASS 0: digit = key >> 21 into hist0 (every element; NaNs are counted in the extra NaN bin as well);
// PASS 1: digit = (key >> 10) & 2047 of the elements whose top 11 bits equal the lo / hi prefix into hist1[lo / hi];
// PASS 2: digit = key & 1023 of the elements whose top 22 bits equal the lo / hi prefix into hist2[lo / hi].
template <int PASS>
__global__ __launch_bounds__(256) void qsel_hist_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ ws) {
  constexpr int NB = PASS == 2 ? 1024 : QS_BINS;
  constexpr int NH = PASS == 0 ? 1 : 2;
  __shared__ unsigned h[NH * NB];
  __shared__ unsigned nan_s;
  unsigned* w = ws + (long)blockIdx.y * QS_WORDS;
  const float* xr = x + (long)blockIdx.y * n;
  for (int i = threadIdx.x; i < NH * NB; i += blockDim.x) h[i] = 0u;
  if (threadIdx.x == 0) nan_s = 0u;
  unsigned pre_lo = 0u, pre_hi = 0u;
  if (PASS > 0) {
    pre_lo = w[QS_STATE + ST_PRE_LO];
    pre_hi = w[QS_STATE + ST_PRE_HI];
  }
  __syncthreads();
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = xr[i];
    const unsigned k = key_of(v);
    if (PASS == 0) {
      atomicAdd(&h[k >> 21], 1u);
      if (v != v) atomicAdd(&nan_s, 1u);
    } else {
      const unsigned top = PASS == 1 ? (k >> 21) : (k >> 10);
      const unsigned d = PASS == 1 ? ((k >> 10) & 2047u) : (k & 1023u);
      if (top == pre_lo) atomicAdd(&h[d], 1u);
      if (top == pre_hi) atomicAdd(&h[NB + d], 1u);
    }
  }
  __syncthreads();
  unsigned* g = w + (PASS == 0 ? QS_H0 : PASS == 1 ? QS_H1 : QS_H2);
  for (int i = threadIdx.x; i < NH * NB; i += blockDim.x) {
    const unsigned c = h[i];
    if (c) atomicAdd(&g[i], c);
  }
  if (PASS == 0 && threadIdx.x == 0 && nan_s) atomicAdd(&w[QS_STATE + ST_NAN], nan_s);
}

// one block per row: the bin that holds each selector's rank, appended to its prefix; the rank within the bin carried on.
// After the last pass the two keys are complete and out[row] = {value lo, value hi} (NaN, NaN if the row holds a NaN).
template <int PASS>
__global__ __launch_bounds__(256) void qsel_pick_kernel(unsigned* __restrict__ ws, unsigned k_lo, unsigned k_hi,
                                                        float* __restrict__ out) {
  constexpr int NB = PASS == 2 ? 1024 : QS_BINS;
  constexpr int PER = NB / 256;  // consecutive bins per thread
  constexpr int SHIFT = PASS == 2 ? 10 : 11;
  __shared__ unsigned part[256];
  __shared__ unsigned res[2];  // new prefix, new rank of the selector in hand
  unsigned* w = ws + (long)blockIdx.x * QS_WORDS;
  unsigned* st = w + QS_STATE;
  unsigned rank[2], pre[2];
  if (PASS == 0) {
    rank[0] = k_lo; rank[1] = k_hi;
    pre[0] = pre[1] = 0u;
  } else {
    rank[0] = st[ST_RANK_LO]; rank[1] = st[ST_RANK_HI];
    pre[0] = st[ST_PRE_LO]; pre[1] = st[ST_PRE_HI];
  }
  unsigned new_pre[2], new_rank[2];
  for (int sidx = 0; sidx < 2; ++sidx) {
    const unsigned* h = w + (PASS == 0 ? QS_H0 : (PASS == 1 ? QS_H1 : QS_H2) + sidx * NB);
    unsigned c[PER], mine = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      c[j] = h[threadIdx.x * PER + j];
      mine += c[j];
    }
    __syncthreads();  // part / res of the previous selector have been read
    part[threadIdx.x] = mine;
    if (threadIdx.x == 0) {
      res[0] = pre[sidx] << SHIFT;  // only reached if the histogram does not cover the rank (never: counts sum to n)
      res[1] = 0u;
    }
    __syncthreads();
    unsigned before = 0u;  // elements in the bins of lower threads (fixed order, exact integers)
    for (int t = 0; t < (int)threadIdx.x; ++t) before += part[t];
    const unsigned r = rank[sidx];
    if (r >= before && r - before < mine) {  // exactly one thread
      unsigned cum = before;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (r >= cum && r - cum < c[j]) {
          res[0] = (pre[sidx] << SHIFT) | (unsigned)(threadIdx.x * PER + j);
          res[1] = r - cum;
        }
        cum += c[j];
      }
    }
    __syncthreads();
    new_pre[sidx] = res[0];
    new_rank[sidx] = res[1];
  }
  if (threadIdx.x == 0) {
    if (PASS < 2) {
      st[ST_PRE_LO] = new_pre[0]; st[ST_PRE_HI] = new_pre[1];
      st[ST_RANK_LO] = new_rank[0]; st[ST_RANK_HI] = new_rank[1];
    } else {
      const bool has_nan = st[ST_NAN] != 0u;
      out[2 * (long)blockIdx.x] = has_nan ? NAN : value_of(new_pre[0]);
      out[2 * (long)blockIdx.x + 1] = has_nan ? NAN : value_of(new_pre[1]);
    }
  }
}

inline int qsel_blocks(int rows, long n) {
  long b = (n + 8191) / 8192;  // >= 32 elements per thread before a block is worth its histogram flush
  long cap = 2048 / rows;
  if (cap < 1) cap = 1;
  if (cap > 1024) cap = 1024;
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

// ---------------------------------------------------------------- fused colour maps
constexpr int TW = 64, TH = 16;            // tile of output pixels per block iteration (4 per thread)
constexpr int HW_T = TW + 2, HH_T = TH + 2;  // with the one-pixel halo

__global__ __launch_bounds__(256) void val_color_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                        int H, int W, int tiles_x, int tiles, int clamp, float kL,
                                                        float kC, float kH, float eps, float* __restrict__ de,
                                                        float* __restrict__ grad, double* __restrict__ part) {
  __shared__ float sL[HH_T * HW_T], sA[HH_T * HW_T], sB[HH_T * HW_T];
  __shared__ double red[16];
  const long HW = (long)H * W;
  const int b = blockIdx.y;
  const float* pb = pred + (long)b * 3 * HW;
  const float* tb = tgt + (long)b * 3 * HW;
  float* deb = de + (long)b * HW;
  float* gb = grad + (long)b * HW;
  double acc = 0.0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    __syncthreads();  // the previous tile's LDS has been read
    for (int e = threadIdx.x; e < HH_T * HW_T; e += blockDim.x) {
      const int y = y0 - 1 + e / HW_T, x = x0 - 1 + e % HW_T;
      float L = 0.f, A = 0.f, Bc = 0.f;  // L = 0 outside the image: F.conv2d(L, K, padding=1)
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const long o = (long)y * W + x;
        float r = pb[o], g = pb[o + HW], bl = pb[o + 2 * HW];
        if (clamp) {
          r = clamp01(r); g = clamp01(g); bl = clamp01(bl);
        }
        rgb_to_lab(r, g, bl, L, A, Bc);
      }
      sL[e] = L;
      sA[e] = A;
      sB[e] = Bc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TH * TW; e += blockDim.x) {
      const int ty = e / TW, tx = e % TW;
      const int y = y0 + ty, x = x0 + tx;
      if (y >= H || x >= W) continue;
      const long o = (long)y * W + x;
      float r = tb[o], g = tb[o + HW], bl = tb[o + 2 * HW];
      if (clamp) {
        r = clamp01(r); g = clamp01(g); bl = clamp01(bl);
      }
      float L2, A2, B2;
      rgb_to_lab(r, g, bl, L2, A2, B2);
      const int c = (ty + 1) * HW_T + tx + 1;
      const float d = ciede2000_metric(sL[c], sA[c], sB[c], L2, A2, B2, kL, kC, kH, eps);
      deb[o] = d;
      acc += (double)d;
      auto at = [&](int dy, int dx) { return sL[c + dy * HW_T + dx]; };
      // cross-correlation with Kx = [[-1,0,1],[-2,0,2],[-1,0,1]], Ky = Kx^T (the expressions of sobel_mag_kernel)
      const float gx = -at(-1, -1) + at(-1, 1) - 2.f * at(0, -1) + 2.f * at(0, 1) - at(1, -1) + at(1, 1);
      const float gy = -at(-1, -1) - 2.f * at(-1, 0) - at(-1, 1) + at(1, -1) + 2.f * at(1, 0) + at(1, 1);
      gb[o] = sqrtf(gx * gx + gy * gy + 1e-12f);
    }
  }
  const double t = block_sum_d(acc, red);
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = t;
}

// out[r] = scale * (part[r][0] + part[r][1] + ...): each thread a fixed strided subsequence, then the block sum
__global__ __launch_bounds__(256) void row_partials_finalize(const double* __restrict__ part, int per_row, double scale,
                                                             double* __restrict__ out) {
  __shared__ double red[16];
  const double* p = part + (long)blockIdx.x * per_row;
  double acc = 0.0;
  for (int i = threadIdx.x; i < per_row; i += blockDim.x) acc += p[i];
  const double t = block_sum_d(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = t * scale;
}

inline int color_blocks(int B, int H, int W) {
  const long tiles = (long)cdiv(H, TH) * cdiv(W, TW);
  long cap = 4096 / B;
  if (cap < 1) cap = 1;
  return (int)(tiles < cap ? tiles : cap);
}

// ---------------------------------------------------------------- masked mean
__global__ __launch_bounds__(256) void masked_sum_kernel(const float* __restrict__ val, const float* __restrict__ key,
                                                         const float* __restrict__ thr, long n, int chunks,
                                                         double* __restrict__ part) {
  __shared__ double red[16];
  const int r = blockIdx.y;
  const long per = (n + chunks - 1) / chunks, i0 = (long)blockIdx.x * per, i1 = min(n, i0 + per);
  const float* v = val + (long)r * n;
  const float* k = key + (long)r * n;
  const float t = thr[r];
  double acc = 0.0, cnt = 0.0;  // the count as a double: exact below 2^53
  for (long i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
    if (k[i] >= t) {
      acc += (double)v[i];
      cnt += 1.0;
    }
  }
  const double s = block_sum_d(acc, red);
  const double c = block_sum_d(cnt, red);
  if (threadIdx.x == 0) {
    part[2 * ((long)r * chunks + blockIdx.x)] = s;
    part[2 * ((long)r * chunks + blockIdx.x) + 1] = c;
  }
}

__global__ __launch_bounds__(256) void masked_finalize(const double* __restrict__ part, int rows, int chunks,
                                                       double* __restrict__ sum, long long* __restrict__ count,
                                                       double* __restrict__ pooled_sum,
                                                       long long* __restrict__ pooled_count) {
  for (int r = threadIdx.x; r < rows; r += blockDim.x) {
    double s = 0.0, c = 0.0;
    for (int j = 0; j < chunks; ++j) {
      s += part[2 * ((long)r * chunks + j)];
      c += part[2 * ((long)r * chunks + j) + 1];
    }
    sum[r] = s;
    count[r] = (long long)c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    long long c = 0;
    for (int r = 0; r < rows; ++r) {
      s += sum[r];
      c += count[r];
    }
    pooled_sum[0] = s;
    pooled_count[0] = c;
  }
}

inline int masked_chunks(int rows, long n) {
  long c = (n + 4095) / 4096;
  long want = (2048 + rows - 1) / rows;
  if (c > want) c = want;
  if (c < 1) c = 1;
  return (int)c;
}

}  // namespace

extern "C" {

size_t nbp_quantile_workspace_bytes(int rows) { return rows > 0 ? (size_t)rows * QS_WORDS * sizeof(unsigned) : 0; }

int nbp_quantile_select(const float* x, int rows, long n, long k_lo, long k_hi, void* ws, float* out, nbp_stream_t s) {
  NBP_REQUIRE(x && ws && out, "nbp_quantile_select: null pointer");
  NBP_REQUIRE(rows > 0 && rows <= 65535, "nbp_quantile_select: rows must be in [1, 65535], got %d", rows);
  NBP_REQUIRE(n >= 1 && n < (1L << 31), "nbp_quantile_select: n must be in [1, 2^31), got %ld", n);
  NBP_REQUIRE(k_lo >= 0 && k_lo <= k_hi && k_hi < n, "nbp_quantile_select: ranks need 0 <= k_lo <= k_hi < n, got %ld %ld",
              k_lo, k_hi);
  unsigned* w = static_cast<unsigned*>(ws);
  if (hipMemsetAsync(w, 0, (size_t)rows * QS_WORDS * sizeof(unsigned), S(s)) != hipSuccess) {
    set_error("nbp_quantile_select: clearing the workspace failed");
    return NBP_ERR_LAUNCH;
  }
  const dim3 grid(qsel_blocks(rows, n), rows);
  qsel_hist_kernel<0><<<grid, 256, 0, S(s)>>>(x, n, w);
  qsel_pick_kernel<0><<<rows, 256, 0, S(s)>>>(w, (unsigned)k_lo, (unsigned)k_hi, out);
  qsel_hist_kernel<1><<<grid, 256, 0, S(s)>>>(x, n, w);
  qsel_pick_kernel<1><<<rows, 256, 0, S(s)>>>(w, 0u, 0u, out);
  qsel_hist_kernel<2><<<grid, 256, 0, S(s)>>>(x, n, w);
  qsel_pick_kernel<2><<<rows, 256, 0, S(s)>>>(w, 0u, 0u, out);
  return check_launch("quantile_select");
}

size_t nbp_val_color_workspace_doubles(int B, int H, int W) {
  return (B > 0 && H > 0 && W > 0) ? (size_t)B * color_blocks(B, H, W) : 0;
}

int nbp_val_color_maps(const float* pred, const float* tgt, int B, int H, int W, int clamp, float kL, float kC, float kH,
                       float eps, double* ws, float* de, float* grad, double* de_mean, nbp_stream_t s) {
  NBP_REQUIRE(pred && tgt && ws && de && grad && de_mean, "nbp_val_color_maps: null pointer");
  NBP_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "nbp_val_color_maps: bad shape %d x 3 x %d x %d", B, H, W);
  NBP_REQUIRE(eps > 0.f, "nbp_val_color_maps: eps must be positive");
  NBP_REQUIRE((long)cdiv(H, TH) * cdiv(W, TW) < (1L << 31), "nbp_val_color_maps: too many tiles");
  const int tiles_x = cdiv(W, TW), tiles = cdiv(H, TH) * tiles_x;
  const int g = color_blocks(B, H, W);
  val_color_kernel<<<dim3(g, B), 256, 0, S(s)>>>(pred, tgt, H, W, tiles_x, tiles, clamp, kL, kC, kH, eps, de, grad, ws);
  row_partials_finalize<<<B, 256, 0, S(s)>>>(ws, g, 1.0 / ((double)H * W), de_mean);
  return check_launch("val_color_maps");
}

size_t nbp_masked_mean_workspace_doubles(int rows, long n) {
  return (rows > 0 && n > 0) ? (size_t)2 * rows * masked_chunks(rows, n) : 0;
}

int nbp_masked_mean(const float* val, const float* key, const float* thr, int rows, long n, double* ws, double* sum,
                    long long* count, double* pooled_sum, long long* pooled_count, nbp_stream_t s) {
  NBP_REQUIRE(val && key && thr && ws && sum && count && pooled_sum && pooled_count, "nbp_masked_mean: null pointer");
  NBP_REQUIRE(rows > 0 && rows <= 65535 && n > 0, "nbp_masked_mean: bad shape %d x %ld", rows, n);
  const int chunks = masked_chunks(rows, n);
  masked_sum_kernel<<<dim3(chunks, rows), 256, 0, S(s)>>>(val, key, thr, n, chunks, ws);
  masked_finalize<<<1, 256, 0, S(s)>>>(ws, rows, chunks, sum, count, pooled_sum, pooled_count);
  return check_launch("masked_mean");
}

}  // extern "C"
