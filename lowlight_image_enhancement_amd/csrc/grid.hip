// Tiled full-frame inference: the validation loop's grids() / grids_inverse() (NAFNet_base/basicsr/models/
// image_restoration_model.py:167-245) on the device.  A frame is cut into overlapping crops of the training size, the
// network runs on the crops, and the overlapping outputs are averaged back.
//
// The plan of one axis (image extent h, crop c <= h; :185-215):  n = (h - 1) / c + 1 tiles, step = c when n == 1, else
// ceil((h - c) / (n - 1) - 1e-8); origins k * step for k < n - 1 and h - c for the last tile.
// With b = n - 1 >= 1 and r = c n - h (0 <= r < c) the numerator is h - c = c b - r and the quotient c - r / b.  Where b
// divides r it is an integer and the double division is exact.  Otherwise its fraction is at least 1 / b, and 1 - r / b
// when r < b; h < 2^31 leaves b < 2^16 or r < c < 2^15 < b, so the fraction is above 2^-16 either way, against 1e-8
// plus at most 2^-22 of rounding in the division.  So step = ceil_div(h - c, n - 1) = c - f, f = r / b in integers,
// for every int extent.  From that form:
//   origin(n - 1) - origin(n - 2) = (c - r) + f (b - 1), which is > 0 and <= c (f b <= r): n strictly increasing
//     origins, every pixel covered;
//   for n >= 3, 2 step >= c + 1 (f <= (c - 1) / 2) and origin(n - 1) - origin(n - 3) - c = (c - r) + f (b - 2) > 0: no
//     pixel is covered by three tiles of one axis.
// Hence at most 2 x 2 tiles cover a pixel, and cover() below finds them in closed form.
//
//   grid_gather   tiles[t - t0][ch][y][x] = img[ch][oi(t) + y][oj(t) + x]                       (bit copies)
//   grid_blend    out[ch][y][x] = (((0 + a) + b) + ...) / count over the covering tiles in ascending t, one fp32 add
//                 at a time and one division: grids_inverse()'s zeros / += per tile / divide by the count map,
//                 operation for operation, so the result is bitwise the reference's.  Pixel-centric: no atomics, no
//                 accumulator or count map in memory, every pixel written once.
// Both are bandwidth kernels: a workgroup walks (plane, row-chunk) items in a grid-stride loop (the item's
// decomposition is uniform, the lanes run along x), 16 bytes per lane where the rows written are 16-byte aligned and,
// in the blend, every tile edge is a multiple of 4 (the rows read may start at any 4-byte address), 4 bytes otherwise.
// Every element offset is 64-bit.
#include <limits.h>

#include "nbp_common.h"

using namespace nbp;

namespace {

struct GAxis {
  int h, c, n, step;
};

bool axis_plan(int h, int c, GAxis* a) {
  if (c < 1 || c > h) return false;
  a->h = h;
  a->c = c;
  a->n = (h - 1) / c + 1;
  a->step = a->n == 1 ? c : (int)(((long)(h - c) + a->n - 2) / (a->n - 1));
  return true;
}

__host__ __device__ __forceinline__ int origin(const GAxis& a, int k) { return k < a.n - 1 ? k * a.step : a.h - a.c; }

// the tiles of one axis that cover coordinate y, ascending: returns their number (1 or 2)
__device__ __forceinline__ int cover(const GAxis& a, int y, int& k0, int& k1) {
  if (a.n == 1) {
    k0 = k1 = 0;
    return 1;
  }
  const int k = min(y / a.step, a.n - 2);                  // the last regular tile that starts at or before y
  const bool lo = k >= 1 && y < (k - 1) * a.step + a.c;    // its predecessor reaches y (then tile k does too)
  const bool mid = y < k * a.step + a.c;
  const bool last = y >= a.h - a.c;                        // the clamped last tile
  k0 = lo ? k - 1 : (mid ? k : a.n - 1);
  k1 = lo ? k : a.n - 1;
  return (int)lo + (int)mid + (int)last;
}

template <int V>
struct Pack {
  float v[V];
};
// 16 bytes at a 4-byte-aligned address (tile columns start anywhere): still one global_load_dwordx4
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
template <int V>
__device__ __forceinline__ Pack<V> ldp(const float* p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const f4u q = *reinterpret_cast<const f4u*>(p);
    r.v[0] = q[0]; r.v[1] = q[1]; r.v[2] = q[2]; r.v[3] = q[3];
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V>
__device__ __forceinline__ void stp(float* p, const Pack<V>& r) {  // V == 4: p is 16-byte aligned
  if constexpr (V == 4) st4(p, make_float4(r.v[0], r.v[1], r.v[2], r.v[3]));
  else *p = r.v[0];
}

// Workgroup shape shared by both kernels: 256 threads = RY rows x TX lanes along x, TX = 1 << txs.  An item is RY (the
// blend) or kGatherU * RY (the gather) rows of one plane, `chunks` items per plane.  A gather thread takes kGatherU
// rows, RY apart, and issues their loads before the first store.  Measured at 2848 x 4256 in 256 x 256 crops: the gather
// (4-byte accesses) at 4.15 TB/s against 2.07 with one row per thread, and 5.1 with 16-byte accesses; the blend, which
// has up to four loads per pixel in flight already, at 134 us with one row against 201 with two (82 VGPRs, 5 waves per
// SIMD instead of 8), and at 169 us with items cut along x as well.
constexpr int kGatherU = 4;

// V == 4: the destination rows are 16-byte aligned (crop_w a multiple of 4), the source columns start anywhere
template <int V>
__global__ __launch_bounds__(256) void grid_gather(const float* __restrict__ img, float* __restrict__ tiles, int C, int H,
                                                   int W, GAxis ai, GAxis aj, int t0, long items, int chunks, int txs) {
  const int xl = threadIdx.x & ((1 << txs) - 1), rl = threadIdx.x >> txs, ry = 256 >> txs, tx = 1 << txs;
  const int cwv = aj.c / V;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long plane = it / chunks;  // (tile - t0) * C + channel
    const int y0 = (int)(it - plane * chunks) * (ry * kGatherU) + rl;
    const long tl = plane / C;
    const int ch = (int)(plane - tl * C);
    const int t = t0 + (int)tl, tr = t / aj.n, tq = t - tr * aj.n;
    const float* src = img + ((long)ch * H + origin(ai, tr)) * W + origin(aj, tq);
    float* dst = tiles + plane * ai.c * aj.c;
    for (int x = xl; x < cwv; x += tx) {
      Pack<V> v[kGatherU];
#pragma unroll
      for (int u = 0; u < kGatherU; ++u) {
        const int y = y0 + u * ry;
        if (y < ai.c) v[u] = ldp<V>(src + (long)y * W + x * V);
      }
#pragma unroll
      for (int u = 0; u < kGatherU; ++u) {
        const int y = y0 + u * ry;
        if (y < ai.c) stp<V>(dst + (long)y * aj.c + x * V, v[u]);
      }
    }
  }
}

// V pixels of row y from column x that share their covering tiles (rows kr[0 .. nr), columns kc[0 .. nc)): the loads
// first, then (((0 + a) + b) + ...) / count in ascending t -- rows first, then columns
template <int V>
__device__ __forceinline__ Pack<V> blend_px(const float* __restrict__ tiles, long plane_of_t0, long t_stride,
                                            const GAxis& ai, const GAxis& aj, int y, int nr, const int (&kr)[2], int x,
                                            int nc, const int (&kc)[2]) {
  Pack<V> v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ri = i >> 1, ci = i & 1;
    if (ri < nr && ci < nc) {
      const long t = (long)kr[ri] * aj.n + kc[ci];
      v[i] = ldp<V>(tiles + plane_of_t0 + t * t_stride + (long)(y - origin(ai, kr[ri])) * aj.c +
                    (x - origin(aj, kc[ci])));
    }
  }
  Pack<V> acc;
#pragma unroll
  for (int e = 0; e < V; ++e) acc.v[e] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if ((i >> 1) < nr && (i & 1) < nc) {
#pragma unroll
      for (int e = 0; e < V; ++e) acc.v[e] = acc.v[e] + v[i].v[e];
    }
  const float cnt = (float)(nr * nc);
#pragma unroll
  for (int e = 0; e < V; ++e) acc.v[e] = acc.v[e] / cnt;
  return acc;
}

// V == 4: W, crop_w and step_j are multiples of 4, so every tile edge is one and a quad shares its covering tiles.
// Frame sizes mostly miss that (2848 x 4256 in 256 x 256 crops: steps 236 / 250) and take V == 1; a variant that loaded
// such quads 16 bytes at a time and did the quads across a tile edge pixel by pixel was slower there (187 us against
// 137: nearly every wave holds one such quad and then runs both paths).
template <int V>
__global__ __launch_bounds__(256) void grid_blend(const float* __restrict__ tiles, float* __restrict__ out, int C, int H,
                                                  int W, GAxis ai, GAxis aj, long items, int chunks, int txs) {
  const int xl = threadIdx.x & ((1 << txs) - 1), rl = threadIdx.x >> txs, ry = 256 >> txs, tx = 1 << txs;
  const int wv = W / V;
  const long tile_plane = (long)ai.c * aj.c, t_stride = tile_plane * C;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int ch = (int)(it / chunks);
    const int y = (int)(it - (long)ch * chunks) * ry + rl;
    if (y >= H) continue;
    int kr[2], kc[2];
    const int nr = cover(ai, y, kr[0], kr[1]);
    float* dst = out + ((long)ch * H + y) * W;
    const long p0 = ch * tile_plane;
    for (int xv = xl; xv < wv; xv += tx) {
      const int x = xv * V;
      const int nc = cover(aj, x, kc[0], kc[1]);
      stp<V>(dst + x, blend_px<V>(tiles, p0, t_stride, ai, aj, y, nr, kr, x, nc, kc));
    }
  }
}

// lanes along x for a row of `xv` accesses: the smallest power of two >= xv, between 8 and 256
int tx_shift(int xv) {
  int s = 3;
  while (s < 8 && (1 << s) < xv) ++s;
  return s;
}

// the plan of (H, W, crop) must be the one the caller passes: the kernels' bounds rest on it
bool same_plan(int H, int W, int crop_h, int crop_w, int n_rows, int step_i, int n_cols, int step_j, GAxis* ai,
               GAxis* aj) {
  return axis_plan(H, crop_h, ai) && axis_plan(W, crop_w, aj) && ai->n == n_rows && ai->step == step_i &&
         aj->n == n_cols && aj->step == step_j;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr long kMaxBlocks = 2048;  // 256 CUs x 8 workgroups: the grid-stride loop takes the rest

}  // namespace

int nbp_grid_plan(int H, int W, int crop_h, int crop_w, int* n_rows, int* step_i, int* n_cols, int* step_j) {
  GAxis ai, aj;
  NBP_REQUIRE(n_rows && step_i && n_cols && step_j, "nbp_grid_plan: null argument");
  NBP_REQUIRE(axis_plan(H, crop_h, &ai) && axis_plan(W, crop_w, &aj),
              "nbp_grid_plan: need 1 <= crop_h <= H and 1 <= crop_w <= W (got H %d W %d crop %d x %d)", H, W, crop_h,
              crop_w);
  *n_rows = ai.n;
  *step_i = ai.step;
  *n_cols = aj.n;
  *step_j = aj.step;
  return NBP_OK;
}

int nbp_grid_gather(const float* img, float* tiles, int C, int H, int W, int crop_h, int crop_w, int n_rows, int step_i,
                    int n_cols, int step_j, int t0, int n, nbp_stream_t s) {
  GAxis ai, aj;
  NBP_REQUIRE(img && tiles, "nbp_grid_gather: null argument");
  NBP_REQUIRE(C >= 1, "nbp_grid_gather: C < 1");
  NBP_REQUIRE(same_plan(H, W, crop_h, crop_w, n_rows, step_i, n_cols, step_j, &ai, &aj),
              "nbp_grid_gather: (n_rows, step_i, n_cols, step_j) is not nbp_grid_plan of this frame and crop");
  const long T = (long)n_rows * n_cols;
  NBP_REQUIRE(T <= INT_MAX && t0 >= 0 && n >= 1 && (long)t0 + n <= T, "nbp_grid_gather: tiles [t0, t0 + n) outside the plan");
  const bool v4 = crop_w % 4 == 0 && aligned16(tiles);
  const int txs = tx_shift(v4 ? crop_w / 4 : crop_w), ry = 256 >> txs;
  const int chunks = cdiv(crop_h, ry * kGatherU);
  const long items = (long)n * C * chunks;
  const unsigned grid = (unsigned)(items < kMaxBlocks ? items : kMaxBlocks);
  if (v4) grid_gather<4><<<grid, 256, 0, S(s)>>>(img, tiles, C, H, W, ai, aj, t0, items, chunks, txs);
  else grid_gather<1><<<grid, 256, 0, S(s)>>>(img, tiles, C, H, W, ai, aj, t0, items, chunks, txs);
  return check_launch("grid_gather");
}

int nbp_grid_blend(const float* tiles, float* out, int C, int H, int W, int crop_h, int crop_w, int n_rows, int step_i,
                   int n_cols, int step_j, nbp_stream_t s) {
  GAxis ai, aj;
  NBP_REQUIRE(tiles && out, "nbp_grid_blend: null argument");
  NBP_REQUIRE(C >= 1, "nbp_grid_blend: C < 1");
  NBP_REQUIRE(same_plan(H, W, crop_h, crop_w, n_rows, step_i, n_cols, step_j, &ai, &aj),
              "nbp_grid_blend: (n_rows, step_i, n_cols, step_j) is not nbp_grid_plan of this frame and crop");
  NBP_REQUIRE((long)n_rows * n_cols <= INT_MAX, "nbp_grid_blend: more than 2^31 - 1 tiles");
  const bool v4 = W % 4 == 0 && crop_w % 4 == 0 && step_j % 4 == 0 && aligned16(out);
  const int txs = tx_shift(v4 ? W / 4 : W), ry = 256 >> txs;
  const int chunks = cdiv(H, ry);
  const long items = (long)C * chunks;
  const unsigned grid = (unsigned)(items < kMaxBlocks ? items : kMaxBlocks);
  if (v4) grid_blend<4><<<grid, 256, 0, S(s)>>>(tiles, out, C, H, W, ai, aj, items, chunks, txs);
  else grid_blend<1><<<grid, 256, 0, S(s)>>>(tiles, out, C, H, W, ai, aj, items, chunks, txs);
  return check_launch("grid_blend");
}
