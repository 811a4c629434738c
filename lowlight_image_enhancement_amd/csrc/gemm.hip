// fp32 MFMA GEMMs for every channel contraction of NAFNet on NHWC activations:
//   the NAFBlock 1x1 convs conv1/conv3/conv4/conv5 (NAFNet_arch.py:31-48), the 2x2/s2 down conv (:106-108,
//   as a GEMM over a space-to-depth gather), the 1x1 up conv + PixelShuffle(2) (:117-122, as a GEMM whose
//   epilogue scatters depth-to-space and adds the skip, :148-149), and their dgrad (the weight gradients: wgrad.hip);
//   and, as the implicit-GEMM mode of the same kernel, the KH x KW convs of the fp32 VGG / AlexNet trunks (conv_f32).
// v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation (one rounding per fma).
#include <cstdint>

#include "nbp_common.h"

using namespace nbp;

namespace {

enum { AM_PLAIN = 0, AM_S2D = 1, AM_SCALE = 2, AM_CONV = 3 };
enum { CM_PLAIN = 0, CM_D2S = 1, CM_RELU = 2, CM_MASK = 3 };

struct GemmP {
  const float* A;
  long lda;
  const float* a_scale;
  int rows_per_img;
  const float* B;
  long ldb;
  float* C;
  long ldc;
  int M, N, K;
  int gh, gw, cs;  // S2D/D2S geometry: low-res grid gh x gw, cs channels per sub-position of the 2x map
  const float* bias;
  const float* R;
  const float* rscale;
  float* pre;
  // AM_CONV (implicit-GEMM KH x KW / stride conv over an NHWC map, zero padded): input ih x iw x cin, output grid
  // gh x gw (rows m = (b, oi, oj)), K index = (ki * kw + kj) * cin + c
  int ih, iw, cin, kh, kw, stride, pad;
};

// offset of element (m, kq*4 .. +3) of a space-to-depth view of a 2x-resolution NHWC map
__device__ __forceinline__ long s2d_off(int m, int k, int gh, int gw, int cs) {
  const int per = gh * gw;
  const int b = m / per, rem = m - b * per;
  const int i = rem / gw, j = rem - i * gw;
  const int q = k / cs, c = k - q * cs;
  const int kh = q >> 1, kw = q & 1;
  return ((long)(b * 2 * gh + 2 * i + kh) * (2 * gw) + 2 * j + kw) * cs + c;
}

template <int BM, int BN, bool B_NK, int AMODE, int CMODE>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmP p) {
  constexpr int BK = 32, LS = BK + 1;
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int A_IT = BM / 32, B_IT = BN / 32;  // float4 loads per thread per K-tile
  __shared__ float As[BM * LS];
  __shared__ float Bs[BN * LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int M = p.M, N = p.N, K = p.K;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[A_IT], rb[B_IT];
  // AM_CONV: each thread's A rows are fixed over the K loop: image origin and top-left input tap of its rows
  long cbase[AM_CONV == AMODE ? A_IT : 1];
  int ci0[AM_CONV == AMODE ? A_IT : 1], cj0[AM_CONV == AMODE ? A_IT : 1];
  if (AMODE == AM_CONV) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int m = m0 + ((tid + it * 256) >> 3);
      const int per = p.gh * p.gw, b = m / per, rem = m - b * per, oi = rem / p.gw, oj = rem - oi * p.gw;
      cbase[it] = (long)b * p.ih * p.iw * p.cin;
      ci0[it] = oi * p.stride - p.pad;
      cj0[it] = oj * p.stride - p.pad;
    }
  }

  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int idx = tid + it * 256;
      const int r = idx >> 3, kq = idx & 7;
      const int m = m0 + r, k = k0 + kq * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < M && k < K) {
        if (AMODE == AM_CONV) {
          const int tap = k / p.cin, c = k - tap * p.cin, ki = tap / p.kw, kj = tap - ki * p.kw;
          const int ii = ci0[it] + ki, jj = cj0[it] + kj;
          if (ii >= 0 && ii < p.ih && jj >= 0 && jj < p.iw)
            v = ld4(p.A + cbase[it] + ((long)ii * p.iw + jj) * p.cin + c);
        } else if (AMODE == AM_S2D) v = ld4(p.A + s2d_off(m, k, p.gh, p.gw, p.cs));
        else v = ld4(p.A + (long)m * p.lda + k);
        if (AMODE == AM_SCALE) v = v * ld4(p.a_scale + (long)(m / p.rows_per_img) * K + k);
      }
      ra[it] = v;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int idx = tid + it * 256;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (B_NK) {
        const int r = idx >> 3, kq = idx & 7;
        const int n = n0 + r, k = k0 + kq * 4;
        if (n < N && k < K) v = ld4(p.B + (long)n * p.ldb + k);
      } else {
        const int kr = idx / (BN / 4), nq = idx % (BN / 4);
        const int k = k0 + kr, n = n0 + nq * 4;
        if (k < K && n < N) v = ld4(p.B + (long)k * p.ldb + n);
      }
      rb[it] = v;
    }
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int idx = tid + it * 256;
      const int r = idx >> 3, kq = idx & 7;
      float* d = As + r * LS + kq * 4;
      d[0] = ra[it].x; d[1] = ra[it].y; d[2] = ra[it].z; d[3] = ra[it].w;
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int idx = tid + it * 256;
      if (B_NK) {
        const int r = idx >> 3, kq = idx & 7;
        float* d = Bs + r * LS + kq * 4;
        d[0] = rb[it].x; d[1] = rb[it].y; d[2] = rb[it].z; d[3] = rb[it].w;
      } else {
        const int kr = idx / (BN / 4), nq = idx % (BN / 4);
        float* d = Bs + (nq * 4) * LS + kr;
        d[0] = rb[it].x; d[LS] = rb[it].y; d[2 * LS] = rb[it].z; d[3 * LS] = rb[it].w;
      }
    }
  };

  const int nk = (K + BK - 1) / BK;
  load_tiles(0);
  store_tiles();
  __syncthreads();
  const int arow = wm * (BM / 2) + (lane & 31);
  const int brow = wn * (BN / 2) + (lane & 31);
  const int kh = lane >> 5;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) load_tiles((t + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[(arow + i * 32) * LS + kk + kh];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[(brow + j * 32) * LS + kk + kh];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    if (t + 1 < nk) {
      store_tiles();
      __syncthreads();
    }
  }

  // epilogue: C/D map of 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
      if (col >= N) continue;
      const float bcol = p.bias ? p.bias[col] : 0.f;
      const float scol = p.rscale ? p.rscale[col] : 1.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= M) continue;
        long off;
        if (CMODE == CM_D2S) off = s2d_off(row, col, p.gh, p.gw, p.cs);
        else off = (long)row * p.ldc + col;
        float v = acc[i][j][r] + bcol;
        if (CMODE == CM_RELU) {
          p.C[off] = fmaxf(v, 0.f);
          continue;
        }
        if (CMODE == CM_MASK) {  // y = acc where R > 0 (the previous post-ReLU map), no bias
          p.C[off] = p.R[off] > 0.f ? acc[i][j][r] : 0.f;
          continue;
        }
        if (p.pre) p.pre[off] = v;
        if (p.R) v = p.R[off] + scol * v;
        p.C[off] = v;
      }
    }
}

template <int BM, int BN, bool B_NK, int AMODE, int CMODE>
void launch_gemm(const GemmP& p, hipStream_t st) {
  dim3 grid(cdiv(p.M, BM), cdiv(p.N, BN));
  gemm_f32_kernel<BM, BN, B_NK, AMODE, CMODE><<<grid, 256, 0, st>>>(p);
}

template <bool B_NK, int AMODE, int CMODE>
void dispatch_tiles(const GemmP& p, hipStream_t st) {
  const bool bn128 = p.N >= 128;
  const long tiles128 = (long)cdiv(p.M, 128) * cdiv(p.N, bn128 ? 128 : 64);
  const bool bm128 = tiles128 >= 1024;
  if (bm128 && bn128) launch_gemm<128, 128, B_NK, AMODE, CMODE>(p, st);
  else if (bm128) launch_gemm<128, 64, B_NK, AMODE, CMODE>(p, st);
  else if (bn128) launch_gemm<64, 128, B_NK, AMODE, CMODE>(p, st);
  else launch_gemm<64, 64, B_NK, AMODE, CMODE>(p, st);
}

}  // namespace

extern "C" {

int nbp_gemm_f32(const float* A, long lda, int a_mode, const float* a_scale, int rows_per_img, const float* B,
                 long ldb, int b_nk, float* C, long ldc, int c_mode, int M, int N, int K, int gh, int gw, int cs,
                 const float* bias, const float* R, const float* rscale, float* pre, nbp_stream_t s) {
  NBP_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "nbp_gemm_f32: null pointer or empty shape");
  NBP_REQUIRE(K % 4 == 0 && N % 4 == 0, "nbp_gemm_f32: K and N must be multiples of 4 (K=%d N=%d)", K, N);
  NBP_REQUIRE(a_mode >= 0 && a_mode <= 2 && c_mode >= 0 && c_mode <= 1, "nbp_gemm_f32: mode");
  NBP_REQUIRE(a_mode != AM_SCALE || (a_scale && rows_per_img > 0), "nbp_gemm_f32: a_scale");
  NBP_REQUIRE((a_mode != AM_S2D && c_mode != CM_D2S) || (gh > 0 && gw > 0 && cs > 0 && cs % 4 == 0),
              "nbp_gemm_f32: s2d geometry");
  NBP_REQUIRE(a_mode != AM_S2D || K == 4 * cs, "nbp_gemm_f32: S2D needs K == 4*cs");
  NBP_REQUIRE(c_mode != CM_D2S || N == 4 * cs, "nbp_gemm_f32: D2S needs N == 4*cs");
  NBP_REQUIRE(a_mode == AM_S2D || lda % 4 == 0, "nbp_gemm_f32: lda alignment");
  GemmP p{A, lda, a_scale, rows_per_img, B, ldb, C, ldc, M, N, K, gh, gw, cs, bias, R, rscale, pre,
          0, 0, 0, 0, 0, 0, 0};
  hipStream_t st = S(s);
  if (b_nk) {
    if (a_mode == AM_PLAIN && c_mode == CM_PLAIN) dispatch_tiles<true, AM_PLAIN, CM_PLAIN>(p, st);
    else if (a_mode == AM_SCALE && c_mode == CM_PLAIN) dispatch_tiles<true, AM_SCALE, CM_PLAIN>(p, st);
    else if (a_mode == AM_S2D && c_mode == CM_PLAIN) dispatch_tiles<true, AM_S2D, CM_PLAIN>(p, st);
    else if (a_mode == AM_PLAIN && c_mode == CM_D2S) dispatch_tiles<true, AM_PLAIN, CM_D2S>(p, st);
    else { set_error("nbp_gemm_f32: unsupported NK mode combination"); return NBP_ERR_ARG; }
  } else {
    if (a_mode == AM_PLAIN && c_mode == CM_PLAIN) dispatch_tiles<false, AM_PLAIN, CM_PLAIN>(p, st);
    else if (a_mode == AM_PLAIN && c_mode == CM_D2S) dispatch_tiles<false, AM_PLAIN, CM_D2S>(p, st);
    else if (a_mode == AM_S2D && c_mode == CM_PLAIN) dispatch_tiles<false, AM_S2D, CM_PLAIN>(p, st);
    else if (a_mode == AM_SCALE && c_mode == CM_PLAIN) dispatch_tiles<false, AM_SCALE, CM_PLAIN>(p, st);
    else { set_error("nbp_gemm_f32: unsupported KN mode combination"); return NBP_ERR_ARG; }
  }
  return check_launch("gemm_f32");
}

}  // extern "C"

namespace nbp {
// fp32 implicit-GEMM convolution (the parity mode of the VGG / LPIPS trunks: the reference's PerceptualLoss runs its
// conv stack in fp32, NewBP_model/losses.py:63-69): y[b][oi][oj][n] = epi(sum_{ki,kj,c} x[b][oi*s+ki-p][oj*s+kj-p][c]
// * w[n][ki*KW+kj][c] (+ bias[n])) on v_mfma_f32_32x32x2_f32 (exact products, fp32 accumulation).
// mode 0 bias + ReLU, 1 bias (or none), 2 ReLU-mask by R (no bias).  Cin, Cout multiples of 4.
int conv_f32(const float* x, int B, int H, int W, int Cin, const float* w, int Cout, int KH, int KW, int stride, int pad,
             const float* bias, int mode, const float* R, float* y, hipStream_t st) {
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  NBP_REQUIRE(Ho > 0 && Wo > 0 && Cin % 4 == 0 && Cout % 4 == 0, "conv_f32: shape");
  const long M = (long)B * Ho * Wo;
  NBP_REQUIRE(M < (1L << 31), "conv_f32: too many pixels");
  const int K = KH * KW * Cin;
  GemmP p{x, 0, nullptr, 1, w, (long)K, y, Cout, (int)M, Cout, K, Ho, Wo, 0, mode == 2 ? nullptr : bias,
          mode == 2 ? R : nullptr, nullptr, nullptr, H, W, Cin, KH, KW, stride, pad};
  if (mode == 0) dispatch_tiles<true, AM_CONV, CM_RELU>(p, st);
  else if (mode == 2) dispatch_tiles<true, AM_CONV, CM_MASK>(p, st);
  else dispatch_tiles<true, AM_CONV, CM_PLAIN>(p, st);
  return check_launch("conv_f32");
}
}  // namespace nbp
