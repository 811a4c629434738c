// SID input path, HBM-resident form: the whole frames stay on the device as uint16 (decoded once), and a batch is
// one gather launch that cuts the crop windows out of them and writes the reference's float32 batch.
//
// Reference: NAFNet_base/basicsr/data/sony_sid_lmdb_dataset.py:162-218 (per sample: crop both frames with one window,
// / 65535, clip(short * ratio, 0, 1), HWC -> CHW).  The crop commutes with the elementwise arithmetic (sid.hip), so
// this is sid_to_float_kernel with a gather in front: sample b reads pixel (top + y, left + x) of its short and of its
// long frame, each through the pointer table with that frame's own row pitch.
//
// Thread mapping: one thread per output pixel, 256 consecutive x per block, one window row per block iteration, the
// three planes written with unit stride along W (a wave stores 256 contiguous bytes per plane).  A window row starts
// at byte 6 * left of a frame row and a frame row is 6 * columns bytes, so nothing wider than 2-byte alignment holds
// for the source: the six samples of a pixel are 2-byte loads (a wave reads one contiguous 384-byte span per frame).
// The launch is bound by its instruction stream as much as by HBM (more rows per thread, or fewer and
// longer-lived blocks, measured slower or equal), so everything uniform over a row -- frame, clamped row, output
// row -- is computed once per block iteration in scalar registers, the frames are addressed as global memory, and
// the division is cheapened:
//
// Arithmetic: bit-identical to numpy's float32 `u / 65535` without the IEEE-division sequence.  With c = fl(1/65535),
// q0 = fl(u * c), r = fma(-q0, 65535, u) (exact) and q = fma(r, c, q0), q equals the correctly rounded quotient for
// every u in [0, 65535] (checked exhaustively in exact arithmetic, and on the device by the all-values case of
// tests/test_gpu_sid_resident.py); q0 alone differs for 512 of them.  Then one rounded multiply by the float32 ratio
// and max / min, as sid_to_float_kernel.
//
// Safety: the host validates the descriptors (data/sony_sid_resident_dataset.py) -- the clamps below are what keeps
// a bug there from reading outside a frame: the frame index is clamped to [0, F), the source row and column to the
// frame, and a frame with no pixels or no pointer reads a zero pixel of the kernel's own.  Rows are walked with a
// grid-stride loop, so a whole-frame window (2848 x 4256) needs no grid.y beyond the limit; every product of sizes
// is 64-bit.
#include "nbp_common.h"

namespace {

// frames are device allocations: global address space (the pointer table alone would give generic "flat" loads)
typedef const __attribute__((address_space(1))) uint16_t* gptr_u16;
__device__ uint16_t g_zero_pixel[4];  // what a frame without pixels or without a pointer reads as

struct FrameRef {
  gptr_u16 p;
  int rows, cols;
};

__device__ __forceinline__ FrameRef frame_ref(const void* const* frames, const int* frame_hw, int idx, int F) {
  const int f = min(max(idx, 0), F - 1);
  FrameRef r;
  r.p = (gptr_u16)frames[f];
  r.rows = frame_hw[2 * f];
  r.cols = frame_hw[2 * f + 1];
  if (!r.p || r.rows <= 0 || r.cols <= 0) {
    r.p = (gptr_u16)g_zero_pixel;
    r.rows = r.cols = 1;
  }
  return r;
}

// first sample of row `row` (clamped into the frame): uniform over the block
__device__ __forceinline__ gptr_u16 row_ptr(const FrameRef& f, long row) {
  const long sy = min(max(row, 0L), (long)f.rows - 1);
  return f.p + sy * f.cols * 3;
}

// offset in samples of column `col` (clamped into the frame; columns * 3 fits an int: the decoder caps them at 2^24)
__device__ __forceinline__ int col_offset(const FrameRef& f, long col) {
  return (int)min(max(col, 0L), (long)f.cols - 1) * 3;
}

// u / 65535 correctly rounded (see the header)
__device__ __forceinline__ float unit16(float u) {
  const float c = 1.0f / 65535.0f;
  const float q0 = u * c;
  return __builtin_fmaf(__builtin_fmaf(-q0, 65535.0f, u), c, q0);
}

__global__ __launch_bounds__(256) void sid_crop_to_float_kernel(const void* const* __restrict__ frames,
                                                                const int* __restrict__ frame_hw,
                                                                const int* __restrict__ desc,
                                                                const float* __restrict__ ratio, int F, int h, int w,
                                                                float* __restrict__ lq, float* __restrict__ sraw,
                                                                float* __restrict__ lraw) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
  if (x >= w) return;
  const int* d = desc + 4 * (long)b;
  const FrameRef fs = frame_ref(frames, frame_hw, d[0], F), fl = frame_ref(frames, frame_hw, d[1], F);
  const long top = d[2], col = (long)d[3] + x;
  const int sx = col_offset(fs, col), lx = col_offset(fl, col);
  const float r = ratio[b];
  const long plane = (long)h * w;
  for (int y = blockIdx.y; y < h; y += gridDim.y) {
    const gptr_u16 srow = row_ptr(fs, top + y), lrow = row_ptr(fl, top + y);
    const long o = (long)b * 3 * plane + (long)y * w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sv = unit16((float)srow[sx + c]);
      const float lv = unit16((float)lrow[lx + c]);
      sraw[o + c * plane + x] = sv;
      lraw[o + c * plane + x] = lv;
      lq[o + c * plane + x] = fminf(fmaxf(sv * r, 0.0f), 1.0f);
    }
  }
}

}  // namespace

extern "C" {

int nbp_sid_crop_to_float(const void* const* frames, const int* frame_hw, const int* desc, const float* ratio, int B,
                          int F, int h, int w, float* lq, float* short_raw, float* long_raw, nbp_stream_t s) {
  NBP_REQUIRE(frames && frame_hw && desc && ratio && lq && short_raw && long_raw && B > 0 && F > 0 && h > 0 && w > 0,
              "nbp_sid_crop_to_float: bad args");
  NBP_REQUIRE(B <= 65535, "nbp_sid_crop_to_float: B <= 65535");
  const dim3 grid((w + 255) / 256, h < 65535 ? h : 65535, B);
  sid_crop_to_float_kernel<<<grid, 256, 0, (hipStream_t)s>>>(frames, frame_hw, desc, ratio, F, h, w, lq, short_raw,
                                                               long_raw);
  return nbp::check_launch("sid_crop_to_float");
}

}  // extern "C"
