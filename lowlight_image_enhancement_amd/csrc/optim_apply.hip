// torch.optim.Adam / AdamW (with or without amsgrad) and torch.optim.SGD steps over the flat fp32 buffers, for the
// train.optim_g kinds of setup_optimizers (image_restoration_model.py:112-142, lowlight_model.py:92-107) beyond the
// plain AdamW of optim.hip.  nbp_optim_prepare has decided everything a step needs and left it in device memory
// (state = {norm, grad multiplier, skip, lr/bc1, sqrt(bc2), lr, S}); these kernels only read it, so a step has no host
// synchronisation and replays from the captured graph.  Order of operations: torch's single-tensor implementations
// (_single_tensor_adam, _single_tensor_sgd), as adamw_kernel follows them for AdamW.
//
// Memory-bound streams: every buffer goes through 16-byte loads and stores (a scalar tail for n % 4), the grid is
// capped at APPLY_MAX_GRID work-groups and strides over the rest.
#include <math.h>

#include "nbp_common.h"

using namespace nbp;

namespace {

constexpr int APPLY_BLOCK = 256;
constexpr int APPLY_MAX_GRID = 2048;  // 256 CUs x 8 work-groups; one pass covers 2048 * 256 * 4 elements

inline int apply_grid(long n) {
  const long g = (n / 4 + APPLY_BLOCK - 1) / APPLY_BLOCK;
  return (int)(g > APPLY_MAX_GRID ? APPLY_MAX_GRID : (g < 1 ? 1 : g));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// omb1 / omb2: 1 - beta formed in double and rounded once, as torch passes `1 - beta` to lerp_ / addcmul_ (1.f - b2
// from the float32 beta2 = 0.999 is off by 1.3e-5 relative: the cancellation keeps beta's rounding error)
struct AdamC {
  float gs, step_size, bc2_sqrt, decay, omb1, b2, omb2, eps, wd;
};

template <bool DECOUPLED, bool AMSGRAD>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, const AdamC& c) {
  g *= c.gs;
  if (DECOUPLED)
    p *= c.decay;  // param.mul_(1 - lr * weight_decay)
  else if (c.wd != 0.f)
    g = g + c.wd * p;  // grad.add(param, alpha=weight_decay)
  m = m + c.omb1 * (g - m);          // exp_avg.lerp_(grad, 1 - beta1)
  v = v * c.b2 + c.omb2 * g * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  float s = v;
  if (AMSGRAD) {
    vmax = fmaxf(vmax, v);
    s = vmax;
  }
  const float denom = sqrtf(s) / c.bc2_sqrt + c.eps;
  p = p - c.step_size * (m / denom);
}

template <bool DECOUPLED, bool AMSGRAD>
__global__ __launch_bounds__(APPLY_BLOCK) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ vmax, long n,
                                                           const float* __restrict__ state, float omb1,
                                                           float b2, float omb2, float eps, float wd) {
  if (state[2] != 0.f) return;  // non-finite gradient: parameters and every buffer untouched (scaler.step skip)
  AdamC c;
  c.gs = state[1];
  c.step_size = state[3];
  c.bc2_sqrt = state[4];
  c.decay = 1.f - state[5] * wd;
  c.omb1 = omb1, c.b2 = b2, c.omb2 = omb2, c.eps = eps, c.wd = wd;
  const long n4 = n / 4;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long i = tid; i < n4; i += stride) {
    float4 pi = ld4(p + 4 * i), mi = ld4(m + 4 * i), vi = ld4(v + 4 * i);
    const float4 gi = ld4(g + 4 * i);
    float4 xi = AMSGRAD ? ld4(vmax + 4 * i) : f4(0.f);
    adam_elem<DECOUPLED, AMSGRAD>(pi.x, gi.x, mi.x, vi.x, xi.x, c);
    adam_elem<DECOUPLED, AMSGRAD>(pi.y, gi.y, mi.y, vi.y, xi.y, c);
    adam_elem<DECOUPLED, AMSGRAD>(pi.z, gi.z, mi.z, vi.z, xi.z, c);
    adam_elem<DECOUPLED, AMSGRAD>(pi.w, gi.w, mi.w, vi.w, xi.w, c);
    st4(p + 4 * i, pi);
    st4(m + 4 * i, mi);
    st4(v + 4 * i, vi);
    if (AMSGRAD) st4(vmax + 4 * i, xi);
  }
  for (long i = 4 * n4 + tid; i < n; i += stride) {  // n % 4 tail
    float pi = p[i], mi = m[i], vi = v[i];
    float xi = AMSGRAD ? vmax[i] : 0.f;
    adam_elem<DECOUPLED, AMSGRAD>(pi, g[i], mi, vi, xi, c);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (AMSGRAD) vmax[i] = xi;
  }
}

struct SgdC {
  float gs, lr, mu, damp1, wd;  // damp1 = 1 - dampening
};

// MODE 0: no momentum; 1: momentum; 2: nesterov.  `first`: the buffer has never been written by an applied step, so
// this one copies the gradient into it (torch: buf = clone(grad), no dampening).
template <int MODE>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, bool first, const SgdC& c) {
  g *= c.gs;
  if (c.wd != 0.f) g = g + c.wd * p;  // grad.add(param, alpha=weight_decay)
  if (MODE != 0) {
    buf = first ? g : buf * c.mu + c.damp1 * g;  // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
    g = MODE == 2 ? g + c.mu * buf : buf;        // grad.add(buf, alpha=momentum) | buf
  }
  p = p - c.lr * g;  // param.add_(grad, alpha=-lr)
}

template <int MODE>
__global__ __launch_bounds__(APPLY_BLOCK) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ buf, long n,
                                                          const float* __restrict__ state,
                                                          const int* __restrict__ ctl, float mu, float damp1,
                                                          float wd) {
  if (state[2] != 0.f) return;  // skipped step: nothing moves, and the buffer stays uninitialised if it was
  // ctl[3] is only read here: sgd_mark_kernel, launched after this kernel on the same stream, writes it
  const bool first = MODE != 0 && ctl[3] == 0;
  SgdC c;
  c.gs = state[1];
  c.lr = state[5];
  c.mu = mu, c.damp1 = damp1, c.wd = wd;
  const long n4 = n / 4;
  const long stride = (long)gridDim.x * blockDim.x;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long i = tid; i < n4; i += stride) {
    float4 pi = ld4(p + 4 * i);
    const float4 gi = ld4(g + 4 * i);
    float4 bi = (MODE != 0 && !first) ? ld4(buf + 4 * i) : f4(0.f);
    sgd_elem<MODE>(pi.x, gi.x, bi.x, first, c);
    sgd_elem<MODE>(pi.y, gi.y, bi.y, first, c);
    sgd_elem<MODE>(pi.z, gi.z, bi.z, first, c);
    sgd_elem<MODE>(pi.w, gi.w, bi.w, first, c);
    st4(p + 4 * i, pi);
    if (MODE != 0) st4(buf + 4 * i, bi);
  }
  for (long i = 4 * n4 + tid; i < n; i += stride) {  // n % 4 tail
    float pi = p[i];
    float bi = (MODE != 0 && !first) ? buf[i] : 0.f;
    sgd_elem<MODE>(pi, g[i], bi, first, c);
    p[i] = pi;
    if (MODE != 0) buf[i] = bi;
  }
}

// One thread, after sgd_kernel: an applied step has initialised the momentum buffer.
__global__ void sgd_mark_kernel(const float* __restrict__ state, int* __restrict__ ctl) {
  if (state[2] == 0.f) ctl[3] = 1;
}

}  // namespace

extern "C" {

int nbp_adam_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long n,
                   const float* state, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                   nbp_stream_t s) {
  NBP_REQUIRE(param && grad && exp_avg && exp_avg_sq && state && n > 0, "nbp_adam_apply: bad args");
  NBP_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) &&
                  aligned16(max_exp_avg_sq),
              "nbp_adam_apply: buffers must be 16-byte aligned");
  const int g = apply_grid(n);
  const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
  const float epsf = (float)eps, wd = (float)weight_decay;
#define NBP_ADAM_LAUNCH(D, A)                                                                                       \
  adam_kernel<D, A><<<g, APPLY_BLOCK, 0, S(s)>>>(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, state, omb1, \
                                                 b2, omb2, epsf, wd)
  if (decoupled) {
    if (max_exp_avg_sq) NBP_ADAM_LAUNCH(true, true); else NBP_ADAM_LAUNCH(true, false);
  } else {
    if (max_exp_avg_sq) NBP_ADAM_LAUNCH(false, true); else NBP_ADAM_LAUNCH(false, false);
  }
#undef NBP_ADAM_LAUNCH
  return check_launch("adam_apply");
}

int nbp_sgd_apply(float* param, const float* grad, float* momentum_buf, long n, const float* state, int* ctl,
                  double momentum, double dampening, double weight_decay, int nesterov, nbp_stream_t s) {
  NBP_REQUIRE(param && grad && state && ctl && n > 0, "nbp_sgd_apply: bad args");
  NBP_REQUIRE((momentum == 0.0) == (momentum_buf == nullptr),
              "nbp_sgd_apply: momentum_buf is needed exactly when momentum != 0");
  NBP_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0),
              "nbp_sgd_apply: nesterov requires momentum > 0 and zero dampening");
  NBP_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(momentum_buf),
              "nbp_sgd_apply: buffers must be 16-byte aligned");
  const int g = apply_grid(n);
  const float mu = (float)momentum, damp1 = (float)(1.0 - dampening), wd = (float)weight_decay;
  if (!momentum_buf) {
    sgd_kernel<0><<<g, APPLY_BLOCK, 0, S(s)>>>(param, grad, nullptr, n, state, ctl, 0.f, 1.f, wd);
    return check_launch("sgd_apply");
  }
  if (nesterov)
    sgd_kernel<2><<<g, APPLY_BLOCK, 0, S(s)>>>(param, grad, momentum_buf, n, state, ctl, mu, damp1, wd);
  else
    sgd_kernel<1><<<g, APPLY_BLOCK, 0, S(s)>>>(param, grad, momentum_buf, n, state, ctl, mu, damp1, wd);
  sgd_mark_kernel<<<1, 1, 0, S(s)>>>(state, ctl);
  return check_launch("sgd_apply");
}

}  // extern "C"
