// Image output, device side: a restored float32 frame becomes PNG scanlines without leaving the device, so one byte
// per sample crosses to the host and the host is left with deflate alone (png_write.cpp).
//
// Reference: NAFNet_base/basicsr/utils/img_util.py:42-104 (tensor2img: clamp, normalise, CHW -> HWC, RGB -> BGR,
// `(img * 255.0).round()`, astype(uint8)); PNG specification sections 6 (filter types) and 9 (filter selection).
//
// img_quantize_kernel.  dst pixel p, channel c is src[(reverse ? C-1-c : c) * N + p] with N = H * W: a [C][N] ->
// [N][C] transpose, so the row structure does not matter.  A thread takes four consecutive pixels: one 16-byte load
// per plane and one 4 * C byte store (a wave reads 1 KiB per plane and writes 768 contiguous bytes for C = 3).  The
// 16-byte loads need every plane 16-byte aligned (src aligned, and N % 4 == 0 when there is more than one plane);
// whatever they cannot cover -- the last N % 4 pixels of one plane, or the whole frame of a source that is only
// 4-byte aligned -- is done one pixel per thread by the same launch.  The arithmetic is tensor2img's in float32 with
// every operation rounded on its own (IEEE division, no reciprocal, no contraction); rintf rounds half to even as
// numpy's round does.  NaN stores 0.
//
// png_filter_kernel.  One workgroup per row.  The raw row and the row above it are staged in LDS behind 16 zero
// bytes each (the `left` / `upper-left` of the first pixel; the row above row 0 is all zero), a thread walks 16-byte
// chunks, and the row is visited twice: once for the five costs (sum of min(b, 256 - b) over the filtered bytes,
// reduced by wave shuffle and then through LDS), once to write the chosen filter.  Rows longer than kLdsRowMax
// bytes are re-read from global memory (and L2) by the same code instead.  A row starts at byte y * W * C of the
// image and at byte y * (W * C + 1) + 1 of the output, so neither is aligned to anything: the 16-byte global
// accesses are declared with alignment 1 (gfx950 runs in unaligned access mode: the compiler keeps them whole).
// No atomics, no workspace; every output byte is written once.
#include <algorithm>

#include "nbp_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ quantiser
__device__ __forceinline__ unsigned quant1(float x, float lo, float hi, float span) {
  float t = fminf(fmaxf(x, lo), hi);
  t = __fdiv_rn(__fsub_rn(t, lo), span);
  const float v = rintf(__fmul_rn(t, 255.0f));
  return x != x ? 0u : (unsigned)v;  // v is in [0, 255] for every other x
}

struct __attribute__((aligned(4))) bytes12 {
  unsigned a, b, c;
};

template <int C>
__global__ __launch_bounds__(256) void img_quantize_kernel(const float* __restrict__ src,
                                                           unsigned char* __restrict__ dst, long N, long nvec,
                                                           float lo, float hi, int reverse) {
  const float span = __fsub_rn(hi, lo);
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  for (long g = tid; g < nvec; g += nth) {  // pixels 4g .. 4g+3
    unsigned q[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 v = nbp::ld4(src + (long)(reverse ? C - 1 - c : c) * N + 4 * g);
      q[c][0] = quant1(v.x, lo, hi, span);
      q[c][1] = quant1(v.y, lo, hi, span);
      q[c][2] = quant1(v.z, lo, hi, span);
      q[c][3] = quant1(v.w, lo, hi, span);
    }
    if constexpr (C == 1) {
      *reinterpret_cast<unsigned*>(dst + 4 * g) = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[0][3] << 24;
    } else {
      bytes12 o;
      o.a = q[0][0] | q[1][0] << 8 | q[2][0] << 16 | q[0][1] << 24;
      o.b = q[1][1] | q[2][1] << 8 | q[0][2] << 16 | q[1][2] << 24;
      o.c = q[2][2] | q[0][3] << 8 | q[1][3] << 16 | q[2][3] << 24;
      *reinterpret_cast<bytes12*>(dst + 12 * g) = o;
    }
  }
  for (long p = 4 * nvec + tid; p < N; p += nth) {
#pragma unroll
    for (int c = 0; c < C; ++c)
      dst[p * C + c] = (unsigned char)quant1(src[(long)(reverse ? C - 1 - c : c) * N + p], lo, hi, span);
  }
}

// ------------------------------------------------------------------------------------------------ PNG filter
constexpr int kLdsRowMax = 32000;  // bytes of one row; 2 * (16 + row rounded up to 16) stays below 64 KiB of LDS
constexpr int kFilterThreads = 256;

// 16 and 4 bytes at any address (one instruction each: see the header)
struct __attribute__((packed)) u128_u {
  unsigned x, y, z, w;
};
struct __attribute__((packed)) u32_u {
  unsigned x;
};

// bytes [i0 - 4, i0 + 16) of a row as five dwords (w[0] = the four bytes before the chunk); i0 is a multiple of 16.
// LDS: the row sits behind 16 zero bytes and is zero-padded to 16, so every chunk is whole.  Global: bytes outside
// [0, L) are not touched and read as zero.
template <bool LDS>
__device__ __forceinline__ void load_chunk(const unsigned char* row, int i0, int L, bool zero, unsigned w[5]) {
  if (LDS) {
    w[0] = *reinterpret_cast<const unsigned*>(row + 16 + i0 - 4);
    const uint4 v = *reinterpret_cast<const uint4*>(row + 16 + i0);
    w[1] = v.x, w[2] = v.y, w[3] = v.z, w[4] = v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = w[4] = 0;
    if (zero) return;
    if (i0 > 0) w[0] = reinterpret_cast<const u32_u*>(row + i0 - 4)->x;
    if (i0 + 16 <= L) {
      const u128_u v = *reinterpret_cast<const u128_u*>(row + i0);
      w[1] = v.x, w[2] = v.y, w[3] = v.z, w[4] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)  // unrolled: w[] stays in registers
        if (i0 + j < L) w[1 + (j >> 2)] |= (unsigned)row[i0 + j] << (8 * (j & 3));
    }
  }
}

__device__ __forceinline__ int byte_of(const unsigned w[5], int j) {  // j in [-4, 16), compile-time after unrolling
  return (int)(w[(j + 4) >> 2] >> (8 * ((j + 4) & 3))) & 255;
}

// the predictor of filter type F (PNG specification 9.2-9.4) from left a, above b, upper-left c
template <int F>
__device__ __forceinline__ int predict(int a, int b, int c) {
  if (F == 0) return 0;
  if (F == 1) return a;
  if (F == 2) return b;
  if (F == 3) return (a + b) >> 1;
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ unsigned cost_of(int f) { return (unsigned)(f < 128 ? f : 256 - f); }

template <int C, bool LDS>
__device__ __forceinline__ void row_costs(const unsigned char* cur, const unsigned char* up, bool up_zero, int L,
                                          unsigned cost[5]) {
  for (int i0 = 16 * threadIdx.x; i0 < L; i0 += 16 * kFilterThreads) {
    unsigned x[5], u[5];
    load_chunk<LDS>(cur, i0, L, false, x);
    load_chunk<LDS>(up, i0, L, up_zero, u);
    const int n = L - i0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int v = byte_of(x, j), a = byte_of(x, j - C), b = byte_of(u, j), c = byte_of(u, j - C);
      const unsigned m = j < n ? 1u : 0u;
      cost[0] += m * cost_of(v);
      cost[1] += m * cost_of((v - predict<1>(a, b, c)) & 255);
      cost[2] += m * cost_of((v - predict<2>(a, b, c)) & 255);
      cost[3] += m * cost_of((v - predict<3>(a, b, c)) & 255);
      cost[4] += m * cost_of((v - predict<4>(a, b, c)) & 255);
    }
  }
}

template <int C, bool LDS, int F>
__device__ __forceinline__ void row_write(const unsigned char* cur, const unsigned char* up, bool up_zero, int L,
                                          unsigned char* out) {
  for (int i0 = 16 * threadIdx.x; i0 < L; i0 += 16 * kFilterThreads) {
    unsigned x[5], u[5], o[4] = {0, 0, 0, 0};
    load_chunk<LDS>(cur, i0, L, false, x);
    load_chunk<LDS>(up, i0, L, up_zero, u);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int f = (byte_of(x, j) - predict<F>(byte_of(x, j - C), byte_of(u, j), byte_of(u, j - C))) & 255;
      o[j >> 2] |= (unsigned)f << (8 * (j & 3));
    }
    if (i0 + 16 <= L) {
      *reinterpret_cast<u128_u*>(out + i0) = u128_u{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (i0 + j < L) out[i0 + j] = (unsigned char)(o[j >> 2] >> (8 * (j & 3)));
    }
  }
}

// global row -> LDS image: 16 zero bytes, the row, zeros up to a multiple of 16
__device__ __forceinline__ void stage_row(const unsigned char* g, bool zero, int L, unsigned char* lds) {
  if (threadIdx.x == 0) *reinterpret_cast<uint4*>(lds) = make_uint4(0, 0, 0, 0);
  for (int i0 = 16 * threadIdx.x; i0 < L; i0 += 16 * kFilterThreads) {
    unsigned w[5];
    load_chunk<false>(g, i0, L, zero, w);
    *reinterpret_cast<uint4*>(lds + 16 + i0) = make_uint4(w[1], w[2], w[3], w[4]);
  }
}

template <int C, bool LDS>
__global__ __launch_bounds__(kFilterThreads) void png_filter_kernel(const unsigned char* __restrict__ img,
                                                                    unsigned char* __restrict__ out, int L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned* red = reinterpret_cast<unsigned*>(smem);  // [4 waves][5] costs, in the first 128 bytes
  const int y = blockIdx.x;
  const unsigned char* cur = img + (long)y * L;
  const unsigned char* up = cur - L;  // never dereferenced for row 0
  const bool up_zero = y == 0;
  if (LDS) {
    const int S = 16 + ((L + 15) & ~15);
    stage_row(cur, false, L, smem + 128);
    stage_row(up, up_zero, L, smem + 128 + S);
    cur = smem + 128;
    up = smem + 128 + S;
    __syncthreads();
  }
  unsigned cost[5] = {0, 0, 0, 0, 0};
  row_costs<C, LDS>(cur, up, LDS ? false : up_zero, L, cost);
#pragma unroll
  for (int f = 0; f < 5; ++f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cost[f] += __shfl_xor(cost[f], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int f = 0; f < 5; ++f) red[(threadIdx.x >> 6) * 5 + f] = cost[f];
  }
  __syncthreads();
  int best = 0;
  unsigned best_cost = 0;
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    unsigned t = 0;
    for (int w = 0; w < kFilterThreads / 64; ++w) t += red[w * 5 + f];
    if (f == 0 || t < best_cost) best = f, best_cost = t;  // ties go to the lowest type
  }
  unsigned char* orow = out + (long)y * (L + 1);
  if (threadIdx.x == 0) orow[0] = (unsigned char)best;
  const bool uz = LDS ? false : up_zero;
  switch (best) {
    case 0: row_write<C, LDS, 0>(cur, up, uz, L, orow + 1); break;
    case 1: row_write<C, LDS, 1>(cur, up, uz, L, orow + 1); break;
    case 2: row_write<C, LDS, 2>(cur, up, uz, L, orow + 1); break;
    case 3: row_write<C, LDS, 3>(cur, up, uz, L, orow + 1); break;
    default: row_write<C, LDS, 4>(cur, up, uz, L, orow + 1); break;
  }
}

template <int C>
void launch_filter(const unsigned char* img, unsigned char* out, int H, int L, hipStream_t st) {
  if (L <= kLdsRowMax) {
    const size_t lds = 128 + 2 * (size_t)(16 + ((L + 15) & ~15));
    png_filter_kernel<C, true><<<H, kFilterThreads, lds, st>>>(img, out, L);
  } else {
    png_filter_kernel<C, false><<<H, kFilterThreads, 128, st>>>(img, out, L);
  }
}

}  // namespace

extern "C" {

int nbp_img_quantize(const float* src, void* dst, int C, int H, int W, float lo, float hi, int reverse,
                     nbp_stream_t s) {
  NBP_REQUIRE(src && dst, "nbp_img_quantize: null pointer");
  NBP_REQUIRE(C == 1 || C == 3, "nbp_img_quantize: C must be 1 or 3, got %d", C);
  NBP_REQUIRE(H >= 1 && W >= 1, "nbp_img_quantize: H and W must be positive, got %d x %d", H, W);
  NBP_REQUIRE(hi > lo, "nbp_img_quantize: min_max needs hi > lo, got (%g, %g)", lo, hi);  // false for NaN too
  NBP_REQUIRE(((uintptr_t)src & 3) == 0, "nbp_img_quantize: src must be 4-byte aligned");
  const long N = (long)H * W;
  const bool vec = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0 && (C == 1 || N % 4 == 0);
  const long nvec = vec ? N / 4 : 0;
  const long items = nvec > N - 4 * nvec ? nvec : N - 4 * nvec;
  const int grid = (int)std::min<long>((items + 255) / 256, 256 * 8);
  if (C == 1)
    img_quantize_kernel<1><<<grid, 256, 0, nbp::S(s)>>>(src, (unsigned char*)dst, N, nvec, lo, hi, reverse != 0);
  else
    img_quantize_kernel<3><<<grid, 256, 0, nbp::S(s)>>>(src, (unsigned char*)dst, N, nvec, lo, hi, reverse != 0);
  return nbp::check_launch("img_quantize");
}

int nbp_png_filter(const void* img, void* out, int H, int W, int C, nbp_stream_t s) {
  NBP_REQUIRE(img && out, "nbp_png_filter: null pointer");
  NBP_REQUIRE(C == 1 || C == 3, "nbp_png_filter: C must be 1 or 3, got %d", C);
  NBP_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 24) && (long)W * C <= (1 << 24),
              "nbp_png_filter: H and W * C must lie within [1, 2^24], got %d x %d x %d", H, W, C);  // 32-bit costs
  const int L = W * C;
  if (C == 1)
    launch_filter<1>((const unsigned char*)img, (unsigned char*)out, H, L, nbp::S(s));
  else
    launch_filter<3>((const unsigned char*)img, (unsigned char*)out, H, L, nbp::S(s));
  return nbp::check_launch("png_filter");
}

}  // extern "C"
