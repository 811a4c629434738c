// Host test of the deferred gradient-reduction queue (csrc/grad_queue.h): queues built from fake, never-dereferenced
// addresses, checked against the rules of its interface.  Built and run by tests/test_grad_queue_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "grad_queue.h"

using namespace nbp;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

// fake address number i: 16-byte aligned, or off by 4 bytes
static float* A(int i) { return reinterpret_cast<float*>((uintptr_t)0x100000 + (uintptr_t)i * 0x1000); }
static float* M4(int i) { return reinterpret_cast<float*>((uintptr_t)0x100000 + (uintptr_t)i * 0x1000 + 4); }

static std::vector<const float*> slabs(const GradQueue& q) {
  std::vector<const float*> v;
  for (const RDesc& d : q.pending()) v.push_back(d.slab);
  return v;
}
static bool same(const RDesc& a, const RDesc& b) {
  return a.slab == b.slab && a.out == b.out && a.L == b.L && a.S == b.S && a.ty == b.ty && a.vec == b.vec &&
         a.blk0 == b.blk0;
}
static bool same(const GradQueue& a, const GradQueue& b) {
  if (a.pending().size() != b.pending().size() || a.post().size() != b.post().size()) return false;
  for (size_t i = 0; i < a.pending().size(); ++i)
    if (!same(a.pending()[i], b.pending()[i])) return false;
  for (size_t i = 0; i < a.post().size(); ++i)
    if (a.post()[i].U != b.post()[i].U || a.post()[i].V != b.post()[i].V) return false;
  return true;
}

// a layer-scale post-op over N x K weights; addresses 50.. are its W, b, scale, dW, db, dscale
static PDesc post(float* U, float* V, int N, int K, int base = 50) {
  return PDesc{U, V, A(base), A(base + 1), A(base + 2), A(base + 3), A(base + 4), A(base + 5), N, K, 0, 0};
}

static void test_make_rdesc() {
  const int S[] = {1, 32, 33, 2048, 2049, 5000}, ty[] = {1, 1, 2, 64, 64, 64};
  for (int i = 0; i < 6; ++i) {
    const RDesc d = make_rdesc(A(0), S[i], 64, A(1));
    CHECK(d.ty == ty[i]);
    CHECK(d.S == S[i] && d.L == 64 && d.slab == A(0) && d.out == A(1) && d.blk0 == 0);
  }
  for (int S2 = 1; S2 <= 5000; ++S2) {  // the smallest power of two with 32 ty >= S, capped at 64
    const int t = make_rdesc(A(0), S2, 4, A(1)).ty;
    CHECK((t & (t - 1)) == 0 && t >= 1 && t <= 64);
    CHECK(t == 64 || 32 * t >= S2);
    CHECK(t == 1 || 32 * (t / 2) < S2);
  }
  CHECK(make_rdesc(A(0), 4, 64, A(1)).vec == 4);
  CHECK(make_rdesc(A(0), 4, 66, A(1)).vec == 1);   // L % 4 != 0
  CHECK(make_rdesc(M4(0), 4, 64, A(1)).vec == 1);  // slab off by 4 bytes
  CHECK(make_rdesc(A(0), 4, 64, M4(1)).vec == 1);  // out off by 4 bytes
  // blocks: (256 / ty) lanes of vec columns each
  CHECK(rdesc_blocks(make_rdesc(A(0), 1, 1024, A(1))) == 1);
  CHECK(rdesc_blocks(make_rdesc(A(0), 1, 1028, A(1))) == 2);
  CHECK(rdesc_blocks(make_rdesc(A(0), 64, 1024, A(1))) == 2);   // ty 2
  CHECK(rdesc_blocks(make_rdesc(A(0), 1, 1022, A(1))) == 4);    // vec 1
}

static void test_plan_flush_rows() {
  const int N = 8, K = 12;
  GradQueue q;
  // post-op 1: U (slab 10 -> out 20) queued before V (11 -> 21); post-op 2: V (13 -> 23) before U (12 -> 22);
  // three unrelated reductions (slabs 1, 2, 3) interleaved
  q.push(A(1), 3, 100, A(31));
  q.push(A(10), 5, (long)N * K, A(20));
  q.push(A(13), 9, N, A(23));
  q.push(A(2), 3, 100, A(32));
  q.push(A(11), 6, N, A(21));
  q.push(A(12), 7, (long)N * K, A(22));
  q.push(A(3), 3, 100, A(33));
  q.push_post(post(A(20), A(21), N, K, 50));
  q.push_post(post(A(22), A(23), N, K, 60));
  std::vector<LDesc> rows;
  std::vector<PDesc> left;
  q.plan_flush(rows, left);
  CHECK(left.empty() && q.post().empty());
  CHECK(rows.size() == 2);
  if (rows.size() == 2) {
    CHECK(rows[0].slabU == A(10) && rows[0].slabV == A(11) && rows[0].SU == 5 && rows[0].SV == 6);
    CHECK(rows[0].W == A(50) && rows[0].b == A(51) && rows[0].scale == A(52) && rows[0].dW == A(53) &&
          rows[0].db == A(54) && rows[0].dscale == A(55) && rows[0].N == N && rows[0].K == K && rows[0].blk0 == 0);
    CHECK(rows[1].slabU == A(12) && rows[1].slabV == A(13) && rows[1].SU == 7 && rows[1].SV == 9);
    CHECK(rows[1].W == A(60) && rows[1].dW == A(63) && rows[1].N == N && rows[1].K == K);
  }
  CHECK((slabs(q) == std::vector<const float*>{A(1), A(2), A(3)}));
}

// one post-op that must stay a post-op; its reductions stay queued
static void stays_post(float* slabU, bool queue_v, int N, int K, long LU, float* W, float* dW) {
  GradQueue q;
  q.push(A(1), 3, 100, A(31));
  q.push(slabU, 5, LU, A(20));
  if (queue_v) q.push(A(11), 6, N, A(21));
  PDesc p = post(A(20), A(21), N, K);
  p.W = W;
  p.dW = dW;
  q.push_post(p);
  GradQueue before = q;
  std::vector<LDesc> rows;
  std::vector<PDesc> left;
  q.plan_flush(rows, left);
  CHECK(rows.empty());
  CHECK(left.size() == 1 && left[0].U == A(20) && left[0].V == A(21) && left[0].W == W && left[0].dW == dW);
  CHECK(q.post().empty());
  CHECK(q.pending().size() == before.pending().size());
  for (size_t i = 0; i < q.pending().size() && i < before.pending().size(); ++i)
    CHECK(same(q.pending()[i], before.pending()[i]));
}

static void test_plan_flush_leftover() {
  stays_post(A(10), false, 8, 12, 8 * 12, A(50), A(53));      // only U queued
  stays_post(A(10), true, 8, 6, 8 * 6, A(50), A(53));         // K = 6
  stays_post(A(10), true, 2, 1028, 2 * 1028, A(50), A(53));   // K = 1028
  stays_post(A(10), true, 8, 12, 8 * 12 + 4, A(50), A(53));   // L_U != N K
  stays_post(M4(10), true, 8, 12, 8 * 12, A(50), A(53));      // U slab off by 4 bytes
  stays_post(A(10), true, 8, 12, 8 * 12, M4(50), A(53));      // W off by 4 bytes
  stays_post(A(10), true, 8, 12, 8 * 12, A(50), M4(53));      // dW off by 4 bytes
  {  // the control: the same queue with nothing wrong becomes a row (K = 1024 is the last K allowed)
    GradQueue q;
    q.push(A(10), 5, 2 * 1024, A(20));
    q.push(A(11), 6, 2, A(21));
    q.push_post(post(A(20), A(21), 2, 1024));
    std::vector<LDesc> rows;
    std::vector<PDesc> left;
    q.plan_flush(rows, left);
    CHECK(rows.size() == 1 && left.empty() && q.pending().empty());
  }
  {  // L_V != N
    GradQueue q;
    q.push(A(10), 5, 8 * 12, A(20));
    q.push(A(11), 6, 9, A(21));
    q.push_post(post(A(20), A(21), 8, 12));
    std::vector<LDesc> rows;
    std::vector<PDesc> left;
    q.plan_flush(rows, left);
    CHECK(rows.empty() && left.size() == 1 && q.pending().size() == 2);
  }
}

static void test_take_direct() {
  for (int b_first = 0; b_first < 2; ++b_first) {  // w and b both queued, b before / after w
    GradQueue q;
    q.push(A(1), 3, 100, A(31));
    q.push(b_first ? A(11) : A(10), 1, b_first ? 8 : 96, b_first ? A(21) : A(20));
    q.push(A(2), 3, 100, A(32));
    q.push(b_first ? A(10) : A(11), 1, b_first ? 96 : 8, b_first ? A(20) : A(21));
    q.push(A(3), 3, 100, A(33));
    q.push_post(post(A(40), A(41), 8, 12));  // an unrelated post-op
    float *ow = nullptr, *ob = nullptr;
    CHECK(q.take_direct(A(10), A(11), &ow, &ob));
    CHECK(ow == A(20) && ob == A(21));
    CHECK((slabs(q) == std::vector<const float*>{A(1), A(2), A(3)}));
    CHECK(q.post().size() == 1);
  }
  {  // w queued, b not
    GradQueue q;
    q.push(A(1), 3, 100, A(31));
    q.push(A(10), 1, 96, A(20));
    GradQueue before = q;
    float *ow = A(70), *ob = A(71);
    CHECK(!q.take_direct(A(10), A(11), &ow, &ob));
    CHECK(same(q, before) && ow == A(70) && ob == A(71));
    CHECK(!q.take_direct(A(12), nullptr, &ow, &ob));  // w not queued
    CHECK(same(q, before) && ow == A(70) && ob == A(71));
  }
  for (int which = 0; which < 2; ++which) {  // w's destination is a post-op's U / b's destination a post-op's V
    GradQueue q;
    q.push(A(10), 1, 96, A(20));
    q.push(A(11), 1, 8, A(21));
    q.push_post(which == 0 ? post(A(20), A(41), 8, 12) : post(A(40), A(21), 8, 12));
    GradQueue before = q;
    float *ow = A(70), *ob = A(71);
    CHECK(!q.take_direct(A(10), A(11), &ow, &ob));
    CHECK(same(q, before) && ow == A(70) && ob == A(71));
  }
  {  // no bias slab: only w removed, even with a reduction of another slab queued around it
    GradQueue q;
    q.push(A(1), 3, 100, A(31));
    q.push(A(10), 1, 96, A(20));
    q.push(A(11), 1, 8, A(21));
    float *ow = nullptr, *ob = A(71);
    CHECK(q.take_direct(A(10), nullptr, &ow, &ob));
    CHECK(ow == A(20) && ob == nullptr);
    CHECK((slabs(q) == std::vector<const float*>{A(1), A(11)}));
  }
  {  // the outputs may alias the inputs (the group launch passes its problem's own slab fields)
    GradQueue q;
    q.push(A(10), 1, 96, A(20));
    q.push(A(11), 1, 8, A(21));
    float *w = A(10), *b = A(11);
    CHECK(q.take_direct(w, b, &w, &b));
    CHECK(w == A(20) && b == A(21) && q.pending().empty());
  }
}

static void test_resplit() {
  GradQueue q;
  q.push(A(10), 40, 96, A(20));
  q.push(A(1), 40, 100, M4(31));
  q.push(A(10), 40, 8, A(21));
  const RDesc other = q.pending()[1];
  q.resplit(A(10), 3);
  CHECK(q.pending().size() == 3);
  const RDesc want0 = make_rdesc(A(10), 3, 96, A(20)), want2 = make_rdesc(A(10), 3, 8, A(21));
  CHECK(want0.ty == 1 && other.ty == 2);
  CHECK(same(q.pending()[0], want0) && same(q.pending()[2], want2));
  CHECK(same(q.pending()[1], other));
  q.resplit(A(10), 100);
  CHECK(q.pending()[0].S == 100 && q.pending()[0].ty == 4 && q.pending()[2].S == 100 && q.pending()[2].ty == 4);
  CHECK(q.pending()[0].vec == 4 && q.pending()[0].L == 96 && q.pending()[0].out == A(20));
  CHECK(same(q.pending()[1], other));
}

static void test_push_clear() {
  GradQueue q;
  CHECK(q.empty());
  q.push(A(1), 3, 100, A(31));
  CHECK(!q.empty() && same(q.pending()[0], make_rdesc(A(1), 3, 100, A(31))));
  q.clear();
  q.push_post(post(A(20), A(21), 8, 12));
  CHECK(!q.empty() && q.pending().empty());
  q.clear();
  CHECK(q.empty());
}

int main() {
  test_make_rdesc();
  test_plan_flush_rows();
  test_plan_flush_leftover();
  test_take_direct();
  test_resplit();
  test_push_clear();
  if (g_fail) std::fprintf(stderr, "grad_queue_test: %d check(s) failed\n", g_fail);
  else std::printf("grad_queue_test: ok\n");
  return g_fail ? 1 : 0;
}
