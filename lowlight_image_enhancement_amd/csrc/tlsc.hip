// TLSC local-window Simplified Channel Attention for full-resolution inference (NAFNetLocal, NAFNet_arch.py:164-174;
// the test-time local converter's AvgPool2d, local_arch.py:29-76, the exact non-fast_imp path).
//
// Where a block's window does not cover its map the SCA's pooled [B][C] vector becomes a per-pixel map.  Four plain
// launches, every element offset 64-bit:
//   tlsc_colsum   cs[b][iv][j][c]  = sum of g over rows iv .. iv + k1 - 1               (fp32, the workspace)
//   tlsc_rowsum   V[b][iv][jv][c]  = sum of cs over columns jv .. jv + k2 - 1 / (k1 k2)
//   tlsc_sca_a    a[p][o]          = b[o] + sum_k W[o][k] V[p][k] at the _h x _w valid positions (fp32 MFMA; reuses
//                                    the workspace)
//   tlsc_gate     ga[b][i][j][c]   = g (.) a[b][clamp(i - pt)][clamp(j - pl)][c], one rounding to g's storage type
// The sliding sums add the entering and subtract the leaving term; each walk is cut into segments of <= 512 outputs
// that start from a freshly summed window, which gives the launches their parallelism along the walked axis and bounds
// the rounding drift of the running sum (<= 1024 roundings at the magnitude of one window sum).
#include "nbp_common.h"

using namespace nbp;

namespace {

template <typename T>
struct Vec {
  static constexpr int N = 16 / sizeof(T);  // channels per 16-byte access
};

template <typename T, int N>
__device__ __forceinline__ void ldv(const T* p, float (&v)[N]) {
  const vec_t<T, N> x = *reinterpret_cast<const vec_t<T, N>*>(p);
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = (float)x[n];
}
template <int N>
__device__ __forceinline__ void stf(float* p, const float (&v)[N]) {
#pragma unroll
  for (int n = 0; n < N; n += 4) st4(p + n, make_float4(v[n], v[n + 1], v[n + 2], v[n + 3]));
}

// vertical pass: thread = 16 bytes of one row position (column x channel group), walks rows [i0, i1) of segment
// blockIdx.y in image blockIdx.z.  rowv = W C / N vectors per row.
template <typename T>
__global__ __launch_bounds__(256) void tlsc_colsum(const T* __restrict__ g, float* __restrict__ cs, int H, long rowv,
                                                   int k1, int hv, int seg) {
  constexpr int N = Vec<T>::N;
  const long x = (long)blockIdx.x * 256 + threadIdx.x;
  if (x >= rowv) return;
  const int i0 = blockIdx.y * seg, i1 = min(hv, i0 + seg);
  const long rs = rowv * N;  // elements per row
  const T* gp = g + ((long)blockIdx.z * H + i0) * rs + x * N;
  float* cp = cs + ((long)blockIdx.z * hv + i0) * rs + x * N;
  float acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.f;
#pragma unroll 4
  for (int r = 0; r < k1; ++r) {
    float v[N];
    ldv<T, N>(gp + r * rs, v);
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] += v[n];
  }
  stf<N>(cp, acc);
#pragma unroll 4
  for (int d = 1; d < i1 - i0; ++d) {  // rows read: i0 + d + k1 - 1 <= hv - 1 + k1 - 1 = H - 1
    float vn[N], vo[N];
    ldv<T, N>(gp + (long)(d + k1 - 1) * rs, vn);
    ldv<T, N>(gp + (long)(d - 1) * rs, vo);
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] += vn[n] - vo[n];
    stf<N>(cp + d * rs, acc);
  }
}

// horizontal pass: thread = one channel quad of one (image, valid row), walks columns [j0, j1) of segment blockIdx.y
__global__ __launch_bounds__(256) void tlsc_rowsum(const float* __restrict__ cs, float* __restrict__ V, long rows, int W,
                                                   int C, int k2, int wv, int seg, float inv) {
  const int Q = C / 4;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * Q) return;
  const long row = t / Q;
  const int q = (int)(t - row * Q);
  const int j0 = blockIdx.y * seg, j1 = min(wv, j0 + seg);
  const float* cp = cs + (row * W + j0) * C + q * 4;
  float* vp = V + (row * wv + j0) * C + q * 4;
  float4 acc = f4(0.f);
#pragma unroll 4
  for (int j = 0; j < k2; ++j) acc += ld4(cp + (long)j * C);
  st4(vp, acc * f4(inv));
#pragma unroll 4
  for (int d = 1; d < j1 - j0; ++d) {  // columns read: j0 + d + k2 - 1 <= wv - 1 + k2 - 1 = W - 1
    acc += ld4(cp + (long)(d + k2 - 1) * C) - ld4(cp + (long)(d - 1) * C);
    st4(vp + (long)d * C, acc * f4(inv));
  }
}

// a[p][o] = b[o] + sum_k W[o][k] V[p][k] over the P valid positions, v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation).  A wave owns 32 positions x 32 NT output channels: D[i = channel][j = position], so a lane ends with
// 4 consecutive channels of one position per accumulator quad (16-byte stores).  The operands want lane <-> row, i.e.
// 64 different cache lines per direct load, so both go through LDS in stages of 32 k: 8 lanes read the 128 contiguous
// bytes of a row (8 lines per wave load; the W stage is shared by the workgroup's 4 waves), the next stage's global
// loads are in flight during this stage's MFMAs.  From LDS a lane reads float4 of 4 consecutive k (lanes 0-31: k = kc ..
// kc + 3, lanes 32-63: kc + 4 .. kc + 7); MFMA u of that chunk takes element u of each, i.e. the k pair (kc + u, kc + 4
// + u) -- the same pairing on both operands, and a sum does not mind the order.  W is streamed in these k stages (it is
// 1 MB at C 512); blockIdx.y walks the 32 NT channel groups.
template <int NT>
__global__ __launch_bounds__(256) void tlsc_sca_a(const float* __restrict__ V, const float* __restrict__ Wm,
                                                  const float* __restrict__ bs, float* __restrict__ a, long P, int C) {
  constexpr int KC = 32;      // k per stage
  constexpr int LS = KC + 4;  // LDS row stride in floats: 144 B puts the 16-byte reads of 16 consecutive rows on distinct banks
  __shared__ __attribute__((aligned(16))) float Ws[32 * NT * LS];
  __shared__ __attribute__((aligned(16))) float Vs[4 * 32 * LS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = ((long)blockIdx.x * 4 + wave) * 32;  // (a wave past P stays for the barriers, fully masked)
  const int o0 = blockIdx.y * (32 * NT);
  const int li = lane & 31, kh = lane >> 5;
  const long p = p0 + li;
  const bool pv = p < P;
  // staging roles: W rows sr + 32 i (i < NT) by the workgroup, V rows vr + 8 i (i < 4) of this wave's 32 positions;
  // k quad sq / vq of the stage
  const int sr = tid >> 3, sq = tid & 7, vr = lane >> 3, vq = lane & 7;
  float4 wreg[NT], vreg[4];
  auto gload = [&](int kk) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int o = o0 + sr + 32 * i, k = kk + 4 * sq;
      wreg[i] = o < C && k < C ? ld4(Wm + (long)o * C + k) : f4(0.f);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long pp = p0 + vr + 8 * i;
      const int k = kk + 4 * vq;
      vreg[i] = pp < P && k < C ? ld4(V + pp * C + k) : f4(0.f);
    }
  };
  floatx16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  gload(0);
  for (int kk = 0; kk < C; kk += KC) {
    __syncthreads();  // the previous stage has been read
#pragma unroll
    for (int i = 0; i < NT; ++i) st4(Ws + (sr + 32 * i) * LS + 4 * sq, wreg[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) st4(Vs + (wave * 32 + vr + 8 * i) * LS + 4 * vq, vreg[i]);
    __syncthreads();
    if (kk + KC < C) gload(kk + KC);
#pragma unroll
    for (int c = 0; c < KC / 8; ++c) {
      if (kk + 8 * c >= C) break;  // (uniform: narrow C)
      const float4 bv = ld4(Vs + (wave * 32 + li) * LS + 8 * c + 4 * kh);
      float4 av[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) av[t] = ld4(Ws + (32 * t + li) * LS + 8 * c + 4 * kh);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(get(av[t], u), get(bv, u), acc[t], 0, 0, 0);
    }
  }
  if (!pv) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int o = o0 + 32 * t + 8 * rq + 4 * kh;  // D row of accumulator r = 4 rq + (r & 3): 8 rq + 4 kh + (r & 3)
      if (o < C)
        st4(a + p * C + o, make_float4(acc[t][4 * rq], acc[t][4 * rq + 1], acc[t][4 * rq + 2], acc[t][4 * rq + 3]) +
                               ld4(bs + o));
    }
}

// gate: thread = 16 bytes of g at (image blockIdx.z, row blockIdx.y, column j, channel group cv); the attention vector
// is gathered from the valid position the replicate padding maps (i, j) to
template <typename T>
__global__ __launch_bounds__(256) void tlsc_gate(const T* __restrict__ g, const float* __restrict__ a, T* __restrict__ ga,
                                                 int H, int W, int C, int hv, int wv, int pt, int pl) {
  constexpr int N = Vec<T>::N;
  const int CV = C / N;
  const long x = (long)blockIdx.x * 256 + threadIdx.x;
  if (x >= (long)W * CV) return;
  const int j = (int)(x / CV), cv = (int)(x - (long)j * CV);
  const int i = blockIdx.y;
  const long b = blockIdx.z;
  const int iv = min(max(i - pt, 0), hv - 1), jv = min(max(j - pl, 0), wv - 1);
  const long off = ((b * H + i) * W + j) * C + cv * N;
  float gv[N], av[N];
  ldv<T, N>(g + off, gv);
  const float* ap = a + ((b * hv + iv) * wv + jv) * C + cv * N;
#pragma unroll
  for (int n = 0; n < N; n += 4) {
    const float4 v = ld4(ap + n);
    av[n] = v.x; av[n + 1] = v.y; av[n + 2] = v.z; av[n + 3] = v.w;
  }
  vec_t<T, N> o;
#pragma unroll
  for (int n = 0; n < N; ++n) o[n] = (T)(gv[n] * av[n]);
  *reinterpret_cast<vec_t<T, N>*>(ga + off) = o;
}

// segment length of a sliding walk over n outputs with a k-term window: enough segments to fill the device given the
// `lanes` independent walks, but each fresh k-term start amortised over >= k / 4 outputs, and never more than 512
int tlsc_seg(long lanes, int n, int k) {
  long nseg = ((1L << 17) + lanes - 1) / lanes;
  if (nseg > n) nseg = n;
  if (nseg < 1) nseg = 1;
  int seg = (int)((n + nseg - 1) / nseg);
  const int lo = (k + 3) / 4 < n ? (k + 3) / 4 : n;
  if (seg < lo) seg = lo;
  if (seg > 512) seg = 512;
  return seg;
}

struct TlscGeo {
  int hv, wv, vseg, hseg;
  long rowv, rows, P;
};

bool tlsc_geo(int B, int H, int W, int C, int k1, int k2, int dtype, TlscGeo* out) {
  if (dtype < 0 || dtype > 2 || B <= 0 || H <= 0 || W <= 0 || C <= 0) return false;
  if (C % (dtype ? 8 : 4) || C > 1024) return false;
  if (k1 < 1 || k1 > H || k2 < 1 || k2 > W) return false;
  if (B > 65535 || H > 65535 || W > (1 << 24)) return false;
  TlscGeo g;
  g.hv = H - k1 + 1;
  g.wv = W - k2 + 1;
  const int N = dtype ? 8 : 4;
  g.rowv = (long)W * C / N;
  g.rows = (long)B * g.hv;
  g.P = g.rows * g.wv;
  g.vseg = tlsc_seg((long)B * g.rowv, g.hv, k1);
  g.hseg = tlsc_seg(g.rows * (C / 4), g.wv, k2);
  const long lim = 1L << 31;
  if (cdiv(g.hv, g.vseg) > 65535 || cdiv(g.wv, g.hseg) > 65535) return false;
  if ((g.rowv + 255) / 256 >= lim || (g.rows * (C / 4) + 255) / 256 >= lim || (g.P + 127) / 128 >= lim) return false;
  *out = g;
  return true;
}

}  // namespace

int nbp_tlsc_supported(int B, int H, int W, int C, int k1, int k2, int dtype) {
  TlscGeo g;
  return tlsc_geo(B, H, W, C, k1, k2, dtype, &g) ? 1 : 0;
}

size_t nbp_tlsc_workspace_bytes(int B, int H, int W, int C, int k1, int k2) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || k1 < 1 || k1 > H || k2 < 1 || k2 > W) return 0;
  return (size_t)B * (size_t)(H - k1 + 1) * (size_t)W * (size_t)C * sizeof(float);  // >= a's [B][_h][_w][C]
}

int nbp_tlsc_pool(const void* g, float* V, void* ws, int B, int H, int W, int C, int k1, int k2, int dtype,
                  nbp_stream_t s) {
  TlscGeo q;
  NBP_REQUIRE(g && V && ws, "nbp_tlsc_pool: null argument");
  NBP_REQUIRE(tlsc_geo(B, H, W, C, k1, k2, dtype, &q), "nbp_tlsc_pool: shape not served (nbp_tlsc_supported)");
  float* cs = static_cast<float*>(ws);
  const dim3 gv((unsigned)((q.rowv + 255) / 256), cdiv(q.hv, q.vseg), B);
  NBP_DISPATCH_T(dtype, tlsc_colsum<T><<<gv, 256, 0, S(s)>>>((const T*)g, cs, H, q.rowv, k1, q.hv, q.vseg));
  if (int rc = check_launch("tlsc_colsum")) return rc;
  const dim3 gh((unsigned)((q.rows * (C / 4) + 255) / 256), cdiv(q.wv, q.hseg));
  tlsc_rowsum<<<gh, 256, 0, S(s)>>>(cs, V, q.rows, W, C, k2, q.wv, q.hseg, 1.f / ((float)k1 * (float)k2));
  return check_launch("tlsc_rowsum");
}

int nbp_tlsc_sca_gate(const void* g, const float* V, const float* wsca, const float* bsca, void* ga, void* ws, int B,
                      int H, int W, int C, int k1, int k2, int dtype, nbp_stream_t s) {
  TlscGeo q;
  NBP_REQUIRE(g && V && wsca && bsca && ga && ws, "nbp_tlsc_sca_gate: null argument");
  NBP_REQUIRE(tlsc_geo(B, H, W, C, k1, k2, dtype, &q), "nbp_tlsc_sca_gate: shape not served (nbp_tlsc_supported)");
  float* a = static_cast<float*>(ws);
  const int nt = C <= 32 ? 1 : (C <= 64 ? 2 : 4);
  const dim3 ga_grid((unsigned)((q.P + 127) / 128), cdiv(C, 32 * nt));
  if (nt == 1) tlsc_sca_a<1><<<ga_grid, 256, 0, S(s)>>>(V, wsca, bsca, a, q.P, C);
  else if (nt == 2) tlsc_sca_a<2><<<ga_grid, 256, 0, S(s)>>>(V, wsca, bsca, a, q.P, C);
  else tlsc_sca_a<4><<<ga_grid, 256, 0, S(s)>>>(V, wsca, bsca, a, q.P, C);
  if (int rc = check_launch("tlsc_sca_a")) return rc;
  const int pt = (H - q.hv) / 2, pl = (W - q.wv) / 2;
  const dim3 gg((unsigned)((q.rowv + 255) / 256), H, B);
  NBP_DISPATCH_T(dtype, tlsc_gate<T><<<gg, 256, 0, S(s)>>>((const T*)g, a, (T*)ga, H, W, C, q.hv, q.wv, pt, pl));
  return check_launch("tlsc_gate");
}
