// The hand-off between the kernels that produce gradient slabs (wgrad.hip and the callers of nbp_reduce_slab /
// nbp_layer_scale_grad) and the flush that reduces them (grad_reduce.hip): the descriptor types and the queue of
// deferred reductions.  Host logic only -- no HIP here, so a plain host compiler builds and tests it
// (tests/host/grad_queue_test.cpp).
//
// Two invariants the queue relies on and does not check:
//  * callers keep every queued slab (and the operands of a queued post-op) alive until the flush;
//  * all flushes of a device are serialised on one stream: the flush's device descriptor table (reduce_table,
//    grad_reduce.hip) is one table per device, written from offset 0 by every flush, so a flush on a second stream
//    overlapping an earlier one would overwrite descriptors that flush is still reading (second item).
#pragma once
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)  // (internal to the library: none of this is exported)
namespace nbp {

// Column sums of a [S][L] fp32 slab into out[L].  Per descriptor: ty row-lanes (each summing <= 32 rows) x (256 / ty)
// lanes of vec columns per block; blk0 = its first block in the launch (set when a launch is packed).
struct RDesc {
  const float* slab;
  float* out;
  long L;
  int S, ty, vec, blk0;
};
// Layer-scale gradient rows reduced straight from the U / V weight-gradient slabs in the same launch (one block per
// row k: U[k][:] = sum_s slabU[s][k][:], V[k] = sum_s slabV[s][k], then the post-op below), so a stage flush is one
// launch and U / V are never written.
struct LDesc {
  const float *slabU, *slabV, *W, *b, *scale;
  float *dW, *db, *dscale;
  int SU, SV, N, K, blk0;
};
// Layer-scale gradient post-op (NAFBlock y = x + beta * conv(h), NAFNet_arch.py:72,80), from U = dOut^T h and
// V = colsum dOut of the UNSCALED output gradient:  dW = s (.) U (rows), db = s (.) V,
// ds[k] = sum_n W[k][n] U[k][n] + b[k] V[k]   (= sum_m dOut[m][k] * conv(h)[m][k]).
struct PDesc {
  const float *U, *V, *W, *b, *scale;
  float *dW, *db, *dscale;
  int N, K, blk0, pad;
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline RDesc make_rdesc(const float* slab, int S, long L, float* out) {
  int ty = 1;
  while (ty < 64 && (long)ty * 32 < S) ty <<= 1;
  const bool v4 = L % 4 == 0 && aligned16(slab) && aligned16(out);
  return RDesc{slab, out, L, S, ty, v4 ? 4 : 1, 0};
}
inline long rdesc_blocks(const RDesc& d) {
  const long per = (long)(256 / d.ty) * d.vec;  // columns per block
  return (d.L + per - 1) / per;
}

// Reductions and post-ops queued while deferral is on, in issue order.
class GradQueue {
 public:
  void push(const float* slab, int S, long L, float* out) { pending_.push_back(make_rdesc(slab, S, L, out)); }
  void push_post(const PDesc& p) { post_.push_back(p); }
  bool empty() const { return pending_.empty() && post_.empty(); }
  void clear() {
    pending_.clear();
    post_.clear();
  }
  const std::vector<RDesc>& pending() const { return pending_; }
  const std::vector<PDesc>& post() const { return post_; }

  // A producer that ends up with ONE split writes its gradient itself: the queued reductions of slab_w (and of slab_b,
  // when non-null) -- copies -- are removed and their destinations returned.  Taken only if every one of them is
  // queued and none feeds a queued post-op (those are reduced straight from the slabs by the flush); otherwise
  // nothing changes.
  bool take_direct(const float* slab_w, const float* slab_b, float** out_w, float** out_b) {
    const int iw = find_slab(slab_w), ib = slab_b ? find_slab(slab_b) : -1;
    if (iw < 0 || feeds_post(pending_[iw].out)) return false;
    if (slab_b && (ib < 0 || feeds_post(pending_[ib].out))) return false;
    *out_w = pending_[iw].out;
    *out_b = slab_b ? pending_[ib].out : nullptr;
    if (ib > iw) pending_.erase(pending_.begin() + ib);  // the higher index first
    pending_.erase(pending_.begin() + iw);
    if (ib >= 0 && ib < iw) pending_.erase(pending_.begin() + ib);
    return true;
  }

  // The producer of `slab` chose S splits after its reduction was queued.
  void resplit(const float* slab, int S) {
    for (RDesc& d : pending_)
      if (d.slab == slab) d.S = S, d.ty = make_rdesc(d.slab, S, d.L, d.out).ty;
  }

  // A post-op whose U and V are both queued reductions becomes a layer-scale row descriptor of the flush's launch
  // (appended to rows) and its two reductions leave the queue, when the row kernel's layout holds: K % 4 == 0,
  // K <= 1024, U of N * K and V of N columns, 16-byte aligned U slab, W and dW.  Every other post-op is appended to
  // leftover_post and runs after the reductions.  The post-ops leave the queue either way.
  void plan_flush(std::vector<LDesc>& rows, std::vector<PDesc>& leftover_post) {
    for (const PDesc& p : post_) {
      const int iu = find_out(p.U), iv = find_out(p.V);
      const bool ok = iu >= 0 && iv >= 0 && p.K % 4 == 0 && p.K <= 1024 && pending_[iu].L == (long)p.N * p.K &&
                      pending_[iv].L == p.N && aligned16(pending_[iu].slab) && aligned16(p.W) && aligned16(p.dW);
      if (!ok) {
        leftover_post.push_back(p);
        continue;
      }
      rows.push_back(LDesc{pending_[iu].slab, pending_[iv].slab, p.W, p.b, p.scale, p.dW, p.db, p.dscale,
                           pending_[iu].S, pending_[iv].S, p.N, p.K, 0});
      pending_.erase(pending_.begin() + (iu > iv ? iu : iv));
      pending_.erase(pending_.begin() + (iu > iv ? iv : iu));
    }
    post_.clear();
  }

 private:
  // the LAST queued reduction reading `slab` / writing `out`, or -1
  int find_slab(const float* slab) const {
    for (int i = (int)pending_.size() - 1; i >= 0; --i)
      if (pending_[i].slab == slab) return i;
    return -1;
  }
  int find_out(const float* out) const {
    for (int i = (int)pending_.size() - 1; i >= 0; --i)
      if (pending_[i].out == out) return i;
    return -1;
  }
  bool feeds_post(const float* out) const {
    for (const PDesc& q : post_)
      if (q.U == out || q.V == out) return true;
    return false;
  }

  std::vector<RDesc> pending_;
  std::vector<PDesc> post_;
};

}  // namespace nbp
#pragma GCC visibility pop
