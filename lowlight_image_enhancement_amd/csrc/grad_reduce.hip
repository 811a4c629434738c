// Reductions of the split-M fp32 gradient slabs (column sums of a [S][L] slab) and the layer-scale gradient post-op.
// While deferral is on for a stream, the reductions issued on it are queued (grad_queue.h) and later executed by ONE
// launch: reduce_multi_kernel (descriptors passed by value in the kernel arguments) or, past one batch,
// reduce_table_kernel (descriptors in a device table); with deferral off a single descriptor is launched at once
// through reduce_multi_kernel (bitwise identical results).  The queue is thread-local.
#include <cstdint>
#include <vector>

#include "nbp_common.h"
#include "grad_queue.h"

using namespace nbp;

namespace {

// Column sums of a [S][L] fp32 slab.  A lane sums VEC adjacent columns (float4 loads when VEC = 4) over the rows
// s = ty (mod TY) with 8 independent accumulators (8 loads in flight), combined in a fixed tree; the TY row-lanes of
// a column are then combined in fixed order through LDS.  Bitwise reproducible.
template <int VEC>
__device__ __forceinline__ void slab_col_partial(const float* __restrict__ base, int S, long L, long col, int ty,
                                                 int TY, float* out) {
  typedef float vf __attribute__((ext_vector_type(VEC)));
  vf a[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) a[u] = (vf)0.f;
  int s = ty;
  for (; s + 7 * TY < S; s += 8 * TY) {
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += *reinterpret_cast<const vf*>(base + (long)(s + u * TY) * L + col);
  }
  for (int u = 0; s < S; s += TY, ++u) a[u & 7] += *reinterpret_cast<const vf*>(base + (long)s * L + col);
  const vf t = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
#pragma unroll
  for (int v = 0; v < VEC; ++v) out[v] = t[v];
}

// out[b][i] = scale * sum_{s < S} slab[b][s][i] (exported batched form; 4 row-lanes x 64 columns per block)
__global__ __launch_bounds__(256) void reduce_slab_kernel(const float* __restrict__ slab, int S, long L, float scale,
                                                          float* __restrict__ out) {
  __shared__ float red[4][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long col = (long)blockIdx.x * 64 + tx;
  float v = 0.f;
  if (col < L) slab_col_partial<1>(slab + (long)blockIdx.y * S * L, S, L, col, ty, 4, &v);
  red[ty][tx] = v;
  __syncthreads();
  if (ty == 0 && col < L) out[(long)blockIdx.y * L + col] = (((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx]) * scale;
}

void launch_reduce(const float* slab, int batch, int S, long L, float scale, float* out, hipStream_t st) {
  reduce_slab_kernel<<<dim3(cdiv(L, 64), batch), 256, 0, st>>>(slab, S, L, scale, out);
}

// ---------------------------------------------------------------- deferred gradient reductions
// One launch's descriptors as the kernels take them, by value: slab reductions (RDesc) in blocks [0, lblk0), then the
// layer-scale rows (LDesc), one block per row.
constexpr int RB_MAX = 48;
constexpr int LB_MAX = 8;
struct RBatch {
  RDesc d[RB_MAX];
  int n;
  LDesc l[LB_MAX];
  int nl, lblk0;
};

__device__ void layer_scale_row_d(const LDesc& d, int lb, float* red) {
  const int row = lb - d.blk0, K = d.K, N = d.N;
  int txq = 1;
  while (txq * 4 < K) txq <<= 1;  // column lanes (4 columns each), a power of two <= 256 (K <= 1024)
  const int TY = 256 / txq, tx = threadIdx.x % txq, ty = threadIdx.x / txq;
  const int col = tx * 4;
  float u[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < K) slab_col_partial<4>(d.slabU + (long)row * K, d.SU, (long)N * K, col, ty, TY, u);
#pragma unroll
  for (int e = 0; e < 4; ++e) red[threadIdx.x * 4 + e] = u[e];
  // V[row]: 256 strided partial sums, folded in fixed order below
  float v = 0.f;
  for (int s2 = threadIdx.x; s2 < d.SV; s2 += 256) v += d.slabV[(long)s2 * N + row];
  __syncthreads();
  const float sc = d.scale[row];
  float dot = 0.f;
  if (ty == 0 && col < K) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int y = 0; y < TY; ++y)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += red[(y * txq + tx) * 4 + e];
    const float4 w = ld4(d.W + (long)row * K + col);
    dot = fmaf(w.x, t[0], fmaf(w.y, t[1], fmaf(w.z, t[2], w.w * t[3])));
    st4(d.dW + (long)row * K + col, make_float4(sc * t[0], sc * t[1], sc * t[2], sc * t[3]));
  }
  __syncthreads();
  red[threadIdx.x] = v;
  red[256 + threadIdx.x] = dot;
  __syncthreads();
  if (threadIdx.x == 0) {
    float vs = 0.f, ds = 0.f;
    for (int i = 0; i < 256; ++i) vs += red[i];
    for (int i = 0; i < txq; ++i) ds += red[256 + i];
    d.dscale[row] = ds + d.b[row] * vs;
    d.db[row] = sc * vs;
  }
}

__device__ void layer_scale_row(const RBatch& rb, int lb, float* red) {
  int j = 0;
  while (j + 1 < rb.nl && rb.l[j + 1].blk0 <= lb) ++j;
  layer_scale_row_d(rb.l[j], lb, red);
}

__device__ void reduce_desc_block(const RDesc& d, int bid, float* red);

__global__ __launch_bounds__(256) void reduce_multi_kernel(RBatch rb) {
  __shared__ float red[256 * 4];
  const int bid = blockIdx.x;
  if (bid >= rb.lblk0) {
    layer_scale_row(rb, bid - rb.lblk0, red);
    return;
  }
  int k = 0;
  while (k + 1 < rb.n && rb.d[k + 1].blk0 <= bid) ++k;
  reduce_desc_block(rb.d[k], bid, red);
}

// one flush as ONE launch: the descriptors in a device table (written by reduce_desc_write from by-value batches, so
// a captured graph replays them), each block's found by binary search on blk0; the same per-descriptor code
__global__ __launch_bounds__(256) void reduce_table_kernel(const RDesc* __restrict__ dd, int n, const LDesc* __restrict__ dl,
                                                           int nl, int lblk0) {
  __shared__ float red[256 * 4];
  const int bid = blockIdx.x;
  if (bid >= lblk0) {
    const int lb = bid - lblk0;
    int lo = 0, hi = nl - 1;  // the last descriptor with blk0 <= lb
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (dl[mid].blk0 <= lb) lo = mid;
      else hi = mid - 1;
    }
    const LDesc d = dl[lo];
    layer_scale_row_d(d, lb, red);
    return;
  }
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (dd[mid].blk0 <= bid) lo = mid;
    else hi = mid - 1;
  }
  const RDesc d = dd[lo];
  reduce_desc_block(d, bid, red);
}

__global__ __launch_bounds__(64) void reduce_desc_write(RBatch rb, RDesc* __restrict__ dd, LDesc* __restrict__ dl) {
  const int t = threadIdx.x;
  if (t < rb.n) dd[t] = rb.d[t];
  if (t < rb.nl) dl[t] = rb.l[t];
}

__device__ void reduce_desc_block(const RDesc& d, int bid, float* red) {
  const int TY = d.ty, TXQ = 256 / TY, VEC = d.vec;
  const int tx = threadIdx.x % TXQ, ty = threadIdx.x / TXQ;
  const long col = ((long)(bid - d.blk0) * TXQ + tx) * VEC;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < d.L) {
    if (VEC == 4) slab_col_partial<4>(d.slab, d.S, d.L, col, ty, TY, v);
    else slab_col_partial<1>(d.slab, d.S, d.L, col, ty, TY, v);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[(ty * TXQ + tx) * 4 + e] = v[e];
  __syncthreads();
  if (ty == 0 && col < d.L) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < TY; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += red[(j * TXQ + tx) * 4 + e];
    if (VEC == 4) st4(d.out + col, make_float4(t[0], t[1], t[2], t[3]));
    else d.out[col] = t[0];
  }
}

// Measurement records of the last call of this thread (nbp_last_call_stats; bench.py's per-launch roofline accounting):
// [0] = slabs + layer-scale rows reduced, [1] = slab bytes read, [2] = bytes written, [3] = reduce_multi_kernel launches
thread_local double g_stats_flush[4];

// the flush's device descriptor table, per device: grown outside graph capture only, never freed (a captured graph
// keeps addressing the table it was captured with); NBP_REDUCE_TABLE=0: the batched launches.  Every flush writes it
// from offset 0: correct only while the flushes of a device are serialised on one stream (grad_queue.h)
bool reduce_table(hipStream_t st, int nd, int nl, RDesc** dd, LDesc** dl) {
  static const bool on = [] {
    const char* e = getenv("NBP_REDUCE_TABLE");
    return !e || atoi(e) != 0;
  }();
  struct Tab { void* p = nullptr; int cd = 0, cl = 0; };
  static Tab tabs[64];
  int dev = 0;
  if (!on || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  Tab& t = tabs[dev];
  if (t.cd < nd || t.cl < nl) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
    const int cd = nd > 4096 ? nd : 4096, cl = nl > 512 ? nl : 512;
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)cd * sizeof(RDesc) + (size_t)cl * sizeof(LDesc)) != hipSuccess) return false;
    t.p = q;  // (the previous table stays allocated)
    t.cd = cd;
    t.cl = cl;
  }
  *dd = reinterpret_cast<RDesc*>(t.p);
  *dl = reinterpret_cast<LDesc*>(reinterpret_cast<char*>(t.p) + (size_t)t.cd * sizeof(RDesc));
  return true;
}

// algorithmic bytes of one descriptor: its slabs read once / its outputs written once
double read_bytes(const RDesc& d) { return (double)d.S * d.L * 4; }
double write_bytes(const RDesc& d) { return (double)d.L * 4; }
double read_bytes(const LDesc& l) { return (double)l.SU * l.N * l.K * 4 + (double)l.SV * l.N * 4; }
double write_bytes(const LDesc& l) { return (double)l.N * (l.K + 2) * 4; }

// The next by-value batch of a flush: descriptors from ds[i] and ls[j] on (both advanced), their blk0 counting on from
// blocks / lblocks (advanced too).  Returns the batch's algorithmic bytes.
double pack_batch(RBatch& rb, const std::vector<RDesc>& ds, size_t& i, long& blocks, const std::vector<LDesc>& ls,
                  size_t& j, int& lblocks) {
  double by = 0;
  rb.n = rb.nl = 0;
  for (; i < ds.size() && rb.n < RB_MAX; ++i) {
    RDesc d = ds[i];
    d.blk0 = (int)blocks;
    blocks += rdesc_blocks(d);
    by += read_bytes(d) + write_bytes(d);
    rb.d[rb.n++] = d;
  }
  for (; j < ls.size() && rb.nl < LB_MAX; ++j) {
    LDesc d = ls[j];
    d.blk0 = lblocks;
    lblocks += d.N;
    by += read_bytes(d) + write_bytes(d);
    rb.l[rb.nl++] = d;
  }
  return by;
}

void launch_multi(const std::vector<RDesc>& ds, hipStream_t st, const std::vector<LDesc>& ls = {}) {
  static const bool log = getenv("NBP_REDUCE_LOG") != nullptr;  // diagnostic: the flush's descriptors to stderr
  double rd = 0, wr = 0;
  for (const RDesc& d : ds) rd += read_bytes(d), wr += write_bytes(d);
  for (const LDesc& l : ls) rd += read_bytes(l), wr += write_bytes(l);
  if (log) {
    fprintf(stderr, "[reduce] flush: %zu slabs + %zu layer-scale, %.2f MB:", ds.size(), ls.size(), rd / 1e6);
    for (const RDesc& d : ds) fprintf(stderr, " %dx%ld", d.S, d.L);
    for (const LDesc& l : ls) fprintf(stderr, " U%dx%dx%d/V%d", l.SU, l.N, l.K, l.SV);
    fprintf(stderr, "\n");
  }
  // measurement record of this flush (nbp_last_call_stats(1, ...))
  g_stats_flush[0] += (double)(ds.size() + ls.size());
  g_stats_flush[1] += rd;
  g_stats_flush[2] += wr;
  RDesc* dd = nullptr;
  LDesc* dl = nullptr;
  size_t i = 0, j = 0;
  long blocks = 0;
  int lblocks = 0;
  if ((ds.size() > (size_t)RB_MAX || ls.size() > (size_t)LB_MAX) &&
      reduce_table(st, (int)ds.size(), (int)ls.size(), &dd, &dl)) {
    // one launch: the descriptors written in by-value batches, blk0 over the whole flush
    double by = 0;
    while (i < ds.size() || j < ls.size()) {
      RBatch rb;
      const size_t i0 = i, j0 = j;
      by += pack_batch(rb, ds, i, blocks, ls, j, lblocks);
      reduce_desc_write<<<1, 64, 0, st>>>(rb, dd + i0, dl + j0);
    }
    lt_begin(st);
    reduce_table_kernel<<<(unsigned)(blocks + lblocks), 256, 0, st>>>(dd, (int)ds.size(), dl, (int)ls.size(),
                                                                       (int)blocks);
    lt_end(st, "reduce_table_kernel", 0.0, by);
    g_stats_flush[3] += 1;
    return;
  }
  while (i < ds.size() || j < ls.size()) {  // one launch per batch, blk0 from 0 in each
    RBatch rb;
    blocks = 0;
    lblocks = 0;
    const double by = pack_batch(rb, ds, i, blocks, ls, j, lblocks);
    rb.lblk0 = (int)blocks;
    lt_begin(st);
    reduce_multi_kernel<<<(unsigned)(blocks + lblocks), 256, 0, st>>>(rb);
    lt_end(st, "reduce_multi_kernel", 0.0, by);
    g_stats_flush[3] += 1;
  }
}

// layer_scale_grad_kernel: one wave per row k; descriptors by value like RBatch; fixed-order wave sum (deterministic)
constexpr int PB_MAX = 24;
struct PBatch {
  PDesc d[PB_MAX];
  int n;
};

__global__ __launch_bounds__(64) void layer_scale_grad_kernel(PBatch pb) {
  const int bid = blockIdx.x;
  int k = 0;
  while (k + 1 < pb.n && pb.d[k + 1].blk0 <= bid) ++k;
  const PDesc& d = pb.d[k];
  const int row = bid - d.blk0, K = d.K, lane = threadIdx.x;
  const float sc = d.scale[row];
  const float* u = d.U + (long)row * K;
  const float* w = d.W + (long)row * K;
  float acc = 0.f;
  for (int i = lane; i < K; i += 64) {
    const float ui = u[i];
    acc = fmaf(w[i], ui, acc);
    d.dW[(long)row * K + i] = sc * ui;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const float v = d.V[row];
    d.dscale[row] = acc + d.b[row] * v;
    d.db[row] = sc * v;
  }
}

void launch_post(const std::vector<PDesc>& ops, hipStream_t st) {
  size_t i = 0;
  while (i < ops.size()) {
    PBatch pb;
    pb.n = 0;
    int blocks = 0;
    for (; i < ops.size() && pb.n < PB_MAX; ++i) {
      PDesc d = ops[i];
      d.blk0 = blocks;
      blocks += d.N;
      pb.d[pb.n++] = d;
    }
    double by = 0;  // U, V, W, b, scale read; dW, db, dscale written
    for (int k = 0; k < pb.n; ++k) by += (double)pb.d[k].N * (2.0 * pb.d[k].K + 4) * 4 + (double)pb.d[k].N * 2 * 4;
    lt_begin(st);
    layer_scale_grad_kernel<<<blocks, 64, 0, st>>>(pb);
    lt_end(st, "layer_scale_grad_kernel", 0.0, by);
  }
}

// this thread's deferred reductions (invariants: grad_queue.h), whether it defers, and the stream of its flushes
thread_local GradQueue g_queue;
thread_local bool g_defer = false;
thread_local hipStream_t g_defer_stream = nullptr;

void flush_pending() {
  for (double& v : g_stats_flush) v = 0;
  // a post-op whose U and V are both reductions of this flush becomes a layer-scale row descriptor of the same launch
  std::vector<LDesc> ls;
  std::vector<PDesc> post;
  g_queue.plan_flush(ls, post);
  launch_multi(g_queue.pending(), g_defer_stream, ls);
  g_queue.clear();
  if (!post.empty()) g_stats_flush[3] += 1;
  launch_post(post, g_defer_stream);  // post-ops read reduction outputs: after every reduction of the flush
}

}  // namespace

namespace nbp {
// scale-1 reduction of a gradient slab: queued while deferral is on (from any stream of this thread: the caller orders
// the flush after every stream that produced a queued slab), launched otherwise
void grad_reduce(const float* slab, int S, long L, float* out, hipStream_t st) {
  if (g_defer) {
    g_queue.push(slab, S, L, out);
    return;
  }
  launch_multi(std::vector<RDesc>{make_rdesc(slab, S, L, out)}, st);
}
bool grad_reduce_deferred() { return g_defer; }
GradQueue& grad_queue() { return g_queue; }
}  // namespace nbp

extern "C" {

int nbp_reduce_slab(const float* slab, int S_, long L, float* out, nbp_stream_t s) {
  NBP_REQUIRE(slab && out && S_ > 0 && L > 0, "nbp_reduce_slab: bad args");
  grad_reduce(slab, S_, L, out, S(s));
  return check_launch("reduce_slab");
}

int nbp_reduce_slab_batched(const float* slab, int batch, int S_, long L, float scale, float* out, nbp_stream_t s) {
  NBP_REQUIRE(slab && out && batch > 0 && batch <= 65535 && S_ > 0 && L > 0, "nbp_reduce_slab_batched: bad args");
  launch_reduce(slab, batch, S_, L, scale, out, S(s));
  return check_launch("reduce_slab_batched");
}

int nbp_layer_scale_grad(const float* U, const float* V, const float* W, const float* b, const float* scale, float* dW,
                         float* db, float* dscale, int N, int K, nbp_stream_t s) {
  NBP_REQUIRE(U && V && W && b && scale && dW && db && dscale && N > 0 && K > 0, "nbp_layer_scale_grad: bad args");
  PDesc d{U, V, W, b, scale, dW, db, dscale, N, K, 0, 0};
  if (g_defer) {
    g_queue.push_post(d);
    return NBP_OK;
  }
  launch_post(std::vector<PDesc>{d}, S(s));
  return check_launch("layer_scale_grad");
}

int nbp_grad_reduce_defer(nbp_stream_t s) {
  NBP_REQUIRE(!g_defer || g_queue.empty() || g_defer_stream == S(s),
              "nbp_grad_reduce_defer: reductions pending on another stream");
  g_defer = true;
  g_defer_stream = S(s);
  return NBP_OK;
}

int nbp_last_call_stats(int which, double* out, int n) {
  NBP_REQUIRE(out && n > 0 && which >= 0 && which <= 2, "nbp_last_call_stats: bad args");
  const double* src = which == 1 ? g_stats_flush : wgrad_stats(which);
  const int len = which == 2 ? 6 : 4;
  for (int i = 0; i < n; ++i) out[i] = i < len ? src[i] : 0.0;
  return NBP_OK;
}

int nbp_grad_reduce_flush(int stop, nbp_stream_t s) {
  NBP_REQUIRE(!g_defer || g_defer_stream == S(s), "nbp_grad_reduce_flush: deferral is active on another stream");
  for (double& v : g_stats_flush) v = 0;
  if (g_defer) flush_pending();
  if (stop) g_defer = false;
  return check_launch("grad_reduce_flush");
}

}  // extern "C"
