// BasicSR pixel losses (NAFNet_base/basicsr/models/losses/losses.py, loss_util.py) on contiguous NCHW fp32 images:
//   L1 |d|, MSE d^2, Charbonnier sqrt(d^2 + eps) with an optional element weight [N][C or 1][H][W] and the reductions
//   'mean' / 'sum' / 'none' of weight_reduce_loss, and PSNRLoss (per-image log of the MSE, optional BT.601 luma).
// The value and the gradient w.r.t. the prediction come out of ONE pass over the inputs: each element is read once,
// its loss goes into a float64 partial and its derivative, already scaled by the upstream gradient, loss_weight and
// the reduction's scale, is stored.  All three kinds are even in d, so d/d target is the same call with the inputs
// swapped.
//
// Access width: every pointer is only guaranteed 4-byte aligned (x.flatten()[1:] is a legal contiguous input).  A
// segment of L elements is split into a scalar head (up to the first 16-byte boundary of its LEAD pointer), a body of
// 4-element groups and a scalar tail.  In the body a pointer that is 16-byte aligned at the head's end moves float4s;
// one that is not (another misalignment than the lead's) moves four dwords.  The choice is uniform over the launch.
// Sums: one float64 partial per work-group (lane order and wave order fixed), combined in index order by a
// one-work-group kernel, so two runs are bitwise equal.
#include <math.h>

#include "nbp_common.h"

using namespace nbp;

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_MAX_BLOCKS = 2048;  // 8 work-groups of 4 waves per CU on 256 CUs

__device__ __forceinline__ int head_of(const float* p, long n) {
  const long h = (long)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
  return (int)(h < n ? h : n);
}
__device__ __forceinline__ bool al16(const float* p) { return ((uintptr_t)p & 15u) == 0; }
__device__ __forceinline__ float4 ldg4(const float* p, bool vec) {
  return vec ? ld4(p) : make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void stg4(float* p, float4 v, bool vec) {
  if (vec) {
    st4(p, v);
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}

// value e and derivative g = de/dd of one element; KIND 0 L1 (sign(0) = 0), 1 MSE, 2 Charbonnier
template <int KIND>
__device__ __forceinline__ void elem(float d, float eps, float& e, float& g) {
  if constexpr (KIND == 0) {
    e = fabsf(d);
    g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  } else if constexpr (KIND == 1) {
    e = d * d;
    g = 2.f * d;
  } else {
    e = sqrtf(d * d + eps);
    g = d / e;
  }
}

struct PixArgs {
  const float* pred;
  const float* target;
  const float* weight;   // null, [N][C][H][W] (wfull) or [N][1][H][W]
  const float* up;       // device scalar, or the upstream map with reduction 'none'; null = 1
  const double* denom;   // weighted mean: the device denominator; null = use inv_n
  float* map;            // reduction 'none': the loss map
  float* grad;           // want_grad: d/d pred
  double* partial;       // mean / sum: one per work-group
  long n, HW, CHW;
  float eps, loss_weight;
  double inv_n;          // 1/n ('mean' without weight) or 1
  int wfull;
};

template <int KIND, bool NONE>
__device__ __forceinline__ void one(const PixArgs& a, long i, float G, double& s) {
  const float d = a.pred[i] - a.target[i];
  float e, g;
  elem<KIND>(d, a.eps, e, g);
  float w = 1.f;
  if (a.weight) w = a.weight[a.wfull ? i : (i / a.CHW) * a.HW + i % a.HW];
  if (a.weight) e *= w;
  if constexpr (NONE) {
    a.map[i] = a.loss_weight * e;
    if (a.grad) a.grad[i] = (a.up ? a.up[i] * G : G) * w * g;
  } else {
    s += (double)e;
    if (a.grad) a.grad[i] = (G * w) * g;
  }
}

// one launch: value partials (mean / sum) or the map (none), and the gradient when a.grad is set
template <int KIND, bool NONE>
__global__ __launch_bounds__(PL_THREADS) void pixel_loss_kernel(PixArgs a) {
  __shared__ double red[16];
  // the gradient's uniform factor: upstream * loss_weight * reduction scale ('none': loss_weight, upstream per element)
  float G = a.loss_weight;
  if constexpr (!NONE) {
    const double u = a.up ? (double)a.up[0] : 1.0;
    G = (float)(a.denom ? u * (double)a.loss_weight / a.denom[0] : u * (double)a.loss_weight * a.inv_n);
  }
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  const int h = head_of(a.pred, a.n);
  const long body = (a.n - h) >> 2, tail0 = h + (body << 2);
  double s = 0.0;
  if (tid < h) one<KIND, NONE>(a, tid, G, s);
  if (tid < a.n - tail0) one<KIND, NONE>(a, tail0 + tid, G, s);
  const bool vt = al16(a.target + h), vg = a.grad && al16(a.grad + h), vm = NONE && al16(a.map + h);
  const bool vu = NONE && a.up && al16(a.up + h);
  // a one-channel weight is addressed per group only when no group straddles a plane: h == 0 and HW % 4 == 0
  const bool wgroup = a.weight && (a.wfull || (h == 0 && (a.HW & 3) == 0));
  for (long q = tid; q < body; q += nth) {
    const long i = h + (q << 2);
    const float4 p = ld4(a.pred + i), t = ldg4(a.target + i, vt);
    float4 w = f4(1.f);
    if (a.weight) {
      if (wgroup) {
        const float* wp = a.weight + (a.wfull ? i : (i / a.CHW) * a.HW + i % a.HW);
        w = ldg4(wp, al16(wp));
      } else {
        w = make_float4(a.weight[(i / a.CHW) * a.HW + i % a.HW], a.weight[((i + 1) / a.CHW) * a.HW + (i + 1) % a.HW],
                        a.weight[((i + 2) / a.CHW) * a.HW + (i + 2) % a.HW],
                        a.weight[((i + 3) / a.CHW) * a.HW + (i + 3) % a.HW]);
      }
    }
    float4 e, g;
    elem<KIND>(p.x - t.x, a.eps, e.x, g.x);
    elem<KIND>(p.y - t.y, a.eps, e.y, g.y);
    elem<KIND>(p.z - t.z, a.eps, e.z, g.z);
    elem<KIND>(p.w - t.w, a.eps, e.w, g.w);
    if (a.weight) e = e * w;
    if constexpr (NONE) {
      stg4(a.map + i, f4(a.loss_weight) * e, vm);
      if (a.grad) {
        const float4 u = a.up ? ldg4(a.up + i, vu) * f4(G) : f4(G);
        stg4(a.grad + i, u * w * g, vg);
      }
    } else {
      s += (double)e.x;
      s += (double)e.y;
      s += (double)e.z;
      s += (double)e.w;
      if (a.grad) stg4(a.grad + i, (f4(G) * w) * g, vg);
    }
  }
  if constexpr (!NONE) {
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
  }
}

// float64 partial sums of x[0..n): the weighted mean's denominator starts here
__global__ __launch_bounds__(PL_THREADS) void sum_partial_kernel(const float* __restrict__ x, long n,
                                                                 double* __restrict__ partial) {
  __shared__ double red[16];
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  const int h = head_of(x, n);
  const long body = (n - h) >> 2, tail0 = h + (body << 2);
  double s = 0.0;
  if (tid < h) s += (double)x[tid];
  if (tid < n - tail0) s += (double)x[tail0 + tid];
  for (long q = tid; q < body; q += nth) {
    const float4 v = ld4(x + h + (q << 2));
    s += (double)v.x;
    s += (double)v.y;
    s += (double)v.z;
    s += (double)v.w;
  }
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one work-group: sum the partials in index order; out_d (denominator) = sum * scale, or
// out_f (loss) = sum * scale [/ denom[0]]
__global__ __launch_bounds__(PL_THREADS) void pixel_finalize_kernel(const double* __restrict__ partial, int np,
                                                                    double scale, const double* __restrict__ denom,
                                                                    double* __restrict__ out_d,
                                                                    float* __restrict__ out_f) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) s += partial[i];
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) {
    if (out_d) out_d[0] = s * scale;
    if (out_f) out_f[0] = (float)(denom ? s * scale / denom[0] : s * scale);
  }
}

// ---------------------------------------------------------------- PSNRLoss
// BT.601 luma of the reference, in its order: the three fp32 products, their left-to-right sum, + 16, / 255 (the
// intrinsics keep the compiler from contracting them into FMAs)
__device__ __forceinline__ float luma(float r, float g, float b) {
  const float s = __fadd_rn(__fadd_rn(__fmul_rn(r, 65.481f), __fmul_rn(g, 128.553f)), __fmul_rn(b, 24.966f));
  return __fadd_rn(s, 16.f) / 255.f;
}

struct PsnrArgs {
  const float* pred;
  const float* target;
  float* grad;          // pass 2
  double* partial;      // [N][bpi] squared-error partials
  const double* coef;   // [N] pass 2: d loss / d mse_n * 2 / M, upstream and loss_weight folded in
  long HW, CHW;         // CHW: the image stride; with toY C == 3
  int bpi;
};

// TOY = false: a segment is one image's C*H*W elements.  TOY = true: a segment is one image's H*W pixels, read from
// three planes of each input and (GRAD) written to three planes.  blockIdx.y = image, blockIdx.x = its bpi chunks.
template <bool TOY, bool GRAD>
__global__ __launch_bounds__(PL_THREADS) void psnr_kernel(PsnrArgs a) {
  __shared__ double red[16];
  const long img = blockIdx.y;
  const float* p = a.pred + img * a.CHW;
  const float* t = a.target + img * a.CHW;
  float* gp = GRAD ? a.grad + img * a.CHW : nullptr;
  const long L = TOY ? a.HW : a.CHW;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  const float k = GRAD ? (float)a.coef[img] : 0.f;
  const float k0 = k * (65.481f / 255.f), k1 = k * (128.553f / 255.f), k2 = k * (24.966f / 255.f);
  double s = 0.0;
  auto scalar = [&](long i) {
    if constexpr (TOY) {
      const float d = luma(p[i], p[a.HW + i], p[2 * a.HW + i]) - luma(t[i], t[a.HW + i], t[2 * a.HW + i]);
      if constexpr (GRAD) {
        gp[i] = k0 * d;
        gp[a.HW + i] = k1 * d;
        gp[2 * a.HW + i] = k2 * d;
      } else {
        s += (double)d * (double)d;
      }
    } else {
      const float d = p[i] - t[i];
      if constexpr (GRAD) {
        gp[i] = k * d;
      } else {
        s += (double)d * (double)d;
      }
    }
  };
  const int h = head_of(p, L);
  const long body = (L - h) >> 2, tail0 = h + (body << 2);
  if (tid < h) scalar(tid);
  if (tid < L - tail0) scalar(tail0 + tid);
  // with toY the planes of one tensor share the lead's alignment only when HW % 4 == 0: decided per plane pointer
  const bool vt = al16(t + h), vg = GRAD && al16(gp + h);
  const bool vp1 = TOY && al16(p + a.HW + h), vp2 = TOY && al16(p + 2 * a.HW + h);
  const bool vt1 = TOY && al16(t + a.HW + h), vt2 = TOY && al16(t + 2 * a.HW + h);
  const bool vg1 = TOY && GRAD && al16(gp + a.HW + h), vg2 = TOY && GRAD && al16(gp + 2 * a.HW + h);
  for (long q = tid; q < body; q += nth) {
    const long i = h + (q << 2);
    float4 d;
    if constexpr (TOY) {
      const float4 pr = ld4(p + i), pg = ldg4(p + a.HW + i, vp1), pb = ldg4(p + 2 * a.HW + i, vp2);
      const float4 tr = ldg4(t + i, vt), tg = ldg4(t + a.HW + i, vt1), tb = ldg4(t + 2 * a.HW + i, vt2);
      d = make_float4(luma(pr.x, pg.x, pb.x) - luma(tr.x, tg.x, tb.x), luma(pr.y, pg.y, pb.y) - luma(tr.y, tg.y, tb.y),
                      luma(pr.z, pg.z, pb.z) - luma(tr.z, tg.z, tb.z), luma(pr.w, pg.w, pb.w) - luma(tr.w, tg.w, tb.w));
    } else {
      d = ld4(p + i) - ldg4(t + i, vt);
    }
    if constexpr (GRAD) {
      if constexpr (TOY) {
        stg4(gp + i, f4(k0) * d, vg);
        stg4(gp + a.HW + i, f4(k1) * d, vg1);
        stg4(gp + 2 * a.HW + i, f4(k2) * d, vg2);
      } else {
        stg4(gp + i, f4(k) * d, vg);
      }
    } else {
      s += (double)d.x * (double)d.x;
      s += (double)d.y * (double)d.y;
      s += (double)d.z * (double)d.z;
      s += (double)d.w * (double)d.w;
    }
  }
  if constexpr (!GRAD) {
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) a.partial[img * a.bpi + blockIdx.x] = s;
  }
}

// one work-group: mse_n = (sum of image n's partials, in index order) / M;
//   loss = loss_weight * 10/ln 10 * mean_n log(mse_n + 1e-8);  coef[n] = up * d loss / d mse_n * 2 / M
__global__ __launch_bounds__(1024) void psnr_finalize_kernel(const double* __restrict__ partial, int N, int bpi,
                                                             double M, double loss_weight,
                                                             const float* __restrict__ up, double* __restrict__ coef,
                                                             float* __restrict__ loss) {
  __shared__ double red[16];
  const double scale = loss_weight * (10.0 / log(10.0)) / (double)N;
  const double u = up ? (double)up[0] : 1.0;
  double s = 0.0;
  if (bpi >= 8) {
    // several partials per image: a wave per image, lane l adds partials l, l + 64, ... and the shuffle tree closes.
    // (A single thread walking a full frame's 2048 partials costs more than the two passes over the frame.)
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int n = threadIdx.x >> 6; n < N; n += nw) {
      double sse = 0.0;
      for (int i = lane; i < bpi; i += 64) sse += partial[(long)n * bpi + i];
      sse = wave_sum_d(sse);
      if (lane == 0) {
        const double mse = sse / M + 1e-8;
        s += log(mse);
        if (coef) coef[n] = u * scale / mse * 2.0 / M;
      }
    }
  } else {
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
      double sse = 0.0;
      for (int i = 0; i < bpi; ++i) sse += partial[(long)n * bpi + i];
      const double mse = sse / M + 1e-8;
      s += log(mse);
      if (coef) coef[n] = u * scale / mse * 2.0 / M;
    }
  }
  s = block_sum_d(s, red);
  if (threadIdx.x == 0 && loss) loss[0] = (float)(scale * s);
}

inline int blocks_for(long n) {
  const long g = ((n + 3) / 4 + PL_THREADS - 1) / PL_THREADS;
  return (int)(g > PL_MAX_BLOCKS ? PL_MAX_BLOCKS : (g < 1 ? 1 : g));
}
inline int psnr_bpi(int N, long L) {
  const int cap = PL_MAX_BLOCKS / N > 0 ? PL_MAX_BLOCKS / N : 1;
  const int g = blocks_for(L);
  return g < cap ? g : cap;
}

template <int KIND>
void launch_pixel(bool none, int g, hipStream_t st, const PixArgs& a) {
  if (none)
    pixel_loss_kernel<KIND, true><<<g, PL_THREADS, 0, st>>>(a);
  else
    pixel_loss_kernel<KIND, false><<<g, PL_THREADS, 0, st>>>(a);
}

}  // namespace

extern "C" {

size_t nbp_pixel_loss_workspace_doubles(long n) { return (size_t)2 * blocks_for(n) + 2; }

int nbp_pixel_loss(const float* pred, const float* target, const float* weight, int N, int C, long HW,
                   int weight_channels, int kind, float eps, int reduction, float loss_weight, int want_grad,
                   const float* up, double* ws, float* out, float* grad, nbp_stream_t s) {
  NBP_REQUIRE(pred && target && out && N > 0 && C > 0 && HW > 0, "nbp_pixel_loss: bad args");
  NBP_REQUIRE(kind >= 0 && kind <= 2 && reduction >= 0 && reduction <= 2, "nbp_pixel_loss: kind 0..2, reduction 0..2");
  NBP_REQUIRE(weight ? (weight_channels == C || weight_channels == 1) : weight_channels == 0,
              "nbp_pixel_loss: weight_channels is C or 1 with a weight, 0 without");
  NBP_REQUIRE(!want_grad || grad, "nbp_pixel_loss: want_grad needs grad");
  NBP_REQUIRE(reduction == 2 || ws, "nbp_pixel_loss: 'mean' and 'sum' need the workspace");
  NBP_REQUIRE((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)weight | (uintptr_t)up | (uintptr_t)out |
                (uintptr_t)grad) & 3) == 0, "nbp_pixel_loss: pointers must be 4-byte aligned");
  const long n = (long)N * C * HW;
  const int g = blocks_for(n);
  const hipStream_t st = S(s);
  PixArgs a{};
  a.pred = pred; a.target = target; a.weight = weight; a.up = up;
  a.map = reduction == 2 ? out : nullptr;
  a.grad = want_grad ? grad : nullptr;
  a.partial = ws;
  a.n = n; a.HW = HW; a.CHW = (long)C * HW;
  a.eps = eps; a.loss_weight = loss_weight;
  a.inv_n = reduction == 0 && !weight ? 1.0 / (double)n : 1.0;
  a.wfull = weight_channels == C;
  if (reduction == 0 && weight) {  // loss_util.py:53-58: weight.sum(), times C for a one-channel weight
    const long nw = (long)N * weight_channels * HW;
    const int gw = blocks_for(nw);
    sum_partial_kernel<<<gw, PL_THREADS, 0, st>>>(weight, nw, ws + g);
    pixel_finalize_kernel<<<1, PL_THREADS, 0, st>>>(ws + g, gw, weight_channels == C ? 1.0 : (double)C, nullptr,
                                                    ws + 2 * g, nullptr);
    a.denom = ws + 2 * g;
  }
  if (kind == 0) launch_pixel<0>(reduction == 2, g, st, a);
  else if (kind == 1) launch_pixel<1>(reduction == 2, g, st, a);
  else launch_pixel<2>(reduction == 2, g, st, a);
  if (reduction != 2)
    pixel_finalize_kernel<<<1, PL_THREADS, 0, st>>>(ws, g, (double)loss_weight * a.inv_n, a.denom, nullptr, out);
  return check_launch("pixel_loss");
}

size_t nbp_psnr_loss_workspace_doubles(int N, int C, long HW, int toY) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (size_t)N * psnr_bpi(N, toY ? HW : (long)C * HW) + (size_t)N;
}

int nbp_psnr_loss(const float* pred, const float* target, int N, int C, long HW, int toY, float loss_weight,
                  int want_grad, const float* up, double* ws, float* loss, float* grad, nbp_stream_t s) {
  NBP_REQUIRE(pred && target && ws && loss && N > 0 && C > 0 && HW > 0, "nbp_psnr_loss: bad args");
  NBP_REQUIRE(N <= 65535, "nbp_psnr_loss: N <= 65535 images");
  NBP_REQUIRE(!toY || C == 3, "nbp_psnr_loss: toY needs three channels");
  NBP_REQUIRE(!want_grad || grad, "nbp_psnr_loss: want_grad needs grad");
  NBP_REQUIRE((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)up | (uintptr_t)grad) & 3) == 0,
              "nbp_psnr_loss: pointers must be 4-byte aligned");
  const long L = toY ? HW : (long)C * HW;
  const int bpi = psnr_bpi(N, L);
  const hipStream_t st = S(s);
  PsnrArgs a{};
  a.pred = pred; a.target = target; a.grad = grad;
  a.partial = ws; a.coef = ws + (long)N * bpi;
  a.HW = HW; a.CHW = (long)C * HW; a.bpi = bpi;
  const dim3 g(bpi, N);
  if (toY) psnr_kernel<true, false><<<g, PL_THREADS, 0, st>>>(a);
  else psnr_kernel<false, false><<<g, PL_THREADS, 0, st>>>(a);
  psnr_finalize_kernel<<<1, 1024, 0, st>>>(ws, N, bpi, (double)L, (double)loss_weight, up,
                                                 want_grad ? ws + (long)N * bpi : nullptr, loss);
  if (want_grad) {
    if (toY) psnr_kernel<true, true><<<g, PL_THREADS, 0, st>>>(a);
    else psnr_kernel<false, true><<<g, PL_THREADS, 0, st>>>(a);
  }
  return check_launch("psnr_loss");
}

}  // extern "C"
