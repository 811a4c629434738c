// Image output, host side: PNG scanlines (the filter kernel's output, imgout.hip) -> a complete PNG file in memory.
//
// Reference: cv2.imwrite behind NAFNet_base/basicsr/utils/img_util.py:147-163.  cv2 / libpng are not in this image;
// the container follows the PNG specification (signature, IHDR, IDAT..., IEND, CRC-32 per chunk) and the zlib stream
// RFC 1950.  Pixel parity with cv2's files is the goal, byte parity is not.
//
// Deflate is parallel in the pigz manner: the scanlines are cut into stripes of whole rows, each stripe is
// raw-deflated on its own (no dictionary carried over) and ends on a byte boundary with Z_FULL_FLUSH, the last with
// Z_FINISH; the zlib stream is the 2-byte header, the stripes in order and the Adler-32 of the whole, combined from
// the stripes' with adler32_combine.  A stripe is about 1 MiB of scanlines and depends on the row length alone, so
// the file does not depend on the number of threads.  Each stripe is one IDAT chunk (the first carries the zlib
// header, the last the Adler-32), and its worker computes that chunk's CRC as well.
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/nbp.h"

namespace nbp {
void set_error(const char* fmt, ...);
}

#define PNGW_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ::nbp::set_error(__VA_ARGS__); \
      return NBP_ERR_ARG;            \
    }                                \
  } while (0)

namespace {

constexpr long kStripeBytes = 1 << 20;
constexpr int kMaxThreads = 256;

inline long stripe_rows(long row_bytes) { return std::max<long>(1, kStripeBytes / row_bytes); }

// what raw deflate of n bytes can grow to at any level (zlib's conservative bound) plus the flush marker
inline long stripe_bound(long n) { return n + ((n + 7) >> 3) + ((n + 63) >> 6) + 5 + 16; }

inline void put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

bool args_ok(int H, int W, int C) { return (C == 1 || C == 3) && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24); }

struct Stripe {
  std::vector<uint8_t> z;  // IDAT payload of this stripe
  uint32_t crc = 0;        // CRC-32 over "IDAT" and the payload
  uint32_t adler = 1;      // Adler-32 of the raw stripe
  int rc = Z_OK;
};

// sequential writer (the caller has checked the total against cap)
struct Sink {
  uint8_t* out;
  long pos = 0;
  void put(const void* p, long n) {
    if (n > 0) memcpy(out + pos, p, (size_t)n);
    pos += n;
  }
  void chunk(const char type[4], const uint8_t* data, uint32_t n, uint32_t crc) {
    uint8_t h[8], t[4];
    put32(h, n);
    memcpy(h + 4, type, 4);
    put32(t, crc);
    put(h, 8);
    put(data, n);
    put(t, 4);
  }
};

}  // namespace

extern "C" {

long nbp_png_encode_bound(int H, int W, int C) {
  if (!args_ok(H, W, C)) {
    ::nbp::set_error("nbp_png_encode_bound: bad shape %d x %d x %d", H, W, C);
    return NBP_ERR_ARG;
  }
  const long row = (long)W * C + 1, per = stripe_rows(row), ns = (H + per - 1) / per;
  const long last = H - (ns - 1) * per;
  return 8 + 25 + 12 + 2 + 4 + ns * 12 + (ns - 1) * stripe_bound(per * row) + stripe_bound(last * row);
}

int nbp_png_encode(const void* scanlines, int H, int W, int C, int level, int nthreads, void* out, long cap,
                   long* len) {
  PNGW_REQUIRE(scanlines && out && len, "nbp_png_encode: null pointer");
  PNGW_REQUIRE(args_ok(H, W, C), "nbp_png_encode: bad shape %d x %d x %d (C is 1 or 3, H and W within [1, 2^24])", H,
               W, C);
  PNGW_REQUIRE(level >= 0 && level <= 9, "nbp_png_encode: level %d outside 0-9", level);
  PNGW_REQUIRE(nthreads >= 1 && nthreads <= kMaxThreads, "nbp_png_encode: nthreads %d outside 1-%d", nthreads,
               kMaxThreads);
  PNGW_REQUIRE(cap >= 0, "nbp_png_encode: negative cap");
  *len = 0;
  const uint8_t* src = (const uint8_t*)scanlines;
  const long row = (long)W * C + 1;
  for (long y = 0; y < H; ++y)
    PNGW_REQUIRE(src[y * row] <= 4, "nbp_png_encode: row %ld has filter type %d (0-4 expected)", y, src[y * row]);

  const long per = stripe_rows(row), ns = (H + per - 1) / per;
  std::vector<Stripe> stripes((size_t)ns);
  // RFC 1950: CMF 0x78 (deflate, 32 KiB window), FLG = the level hint with the check bits
  const uint8_t zhdr[2] = {0x78, (uint8_t)(level <= 1 ? 0x01 : level <= 5 ? 0x5e : level == 6 ? 0x9c : 0xda)};
  std::atomic<long> next{0};
  auto work = [&]() {
    for (long i; (i = next.fetch_add(1)) < ns;) {
      Stripe& st = stripes[(size_t)i];
      const long y0 = i * per, rows = std::min<long>(per, H - y0), n = rows * row;
      const uint8_t* p = src + y0 * row;
      const long head = i == 0 ? 2 : 0;
      z_stream zs;
      memset(&zs, 0, sizeof(zs));
      if ((st.rc = deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY)) != Z_OK) continue;
      st.z.resize((size_t)(head + std::max<long>(stripe_bound(n), (long)deflateBound(&zs, (uLong)n) + 16)));
      if (head) memcpy(st.z.data(), zhdr, 2);
      zs.next_in = const_cast<Bytef*>(p);
      zs.avail_in = (uInt)n;  // rows are at most 3 * 2^24 + 1 bytes
      zs.next_out = st.z.data() + head;
      zs.avail_out = (uInt)(st.z.size() - head);
      const bool fin = i == ns - 1;
      const int z = deflate(&zs, fin ? Z_FINISH : Z_FULL_FLUSH);
      st.rc = (fin ? z == Z_STREAM_END : (z == Z_OK && zs.avail_in == 0 && zs.avail_out > 0)) ? Z_OK : Z_BUF_ERROR;
      st.z.resize((size_t)(head + zs.total_out));
      deflateEnd(&zs);
      st.adler = (uint32_t)adler32(adler32(0, nullptr, 0), p, (uInt)n);
      st.crc = (uint32_t)crc32(crc32(crc32(0, nullptr, 0), (const Bytef*)"IDAT", 4), st.z.data(), (uInt)st.z.size());
    }
  };
  const int nt = (int)std::min<long>(nthreads, ns);
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  for (long i = 0; i < ns; ++i)
    PNGW_REQUIRE(stripes[(size_t)i].rc == Z_OK, "nbp_png_encode: deflate failed on stripe %ld (zlib %d)", i,
                 stripes[(size_t)i].rc);

  uint32_t adler = 1;
  for (long i = 0; i < ns; ++i) {
    const long rows = std::min<long>(per, H - i * per);
    adler = (uint32_t)adler32_combine(adler, stripes[(size_t)i].adler, (z_off_t)(rows * row));
  }
  Stripe& tail = stripes[(size_t)(ns - 1)];
  uint8_t ad[4];
  put32(ad, adler);
  tail.z.insert(tail.z.end(), ad, ad + 4);
  tail.crc = (uint32_t)crc32(tail.crc, ad, 4);

  long need = 8 + 25 + 12;
  for (const Stripe& st : stripes) need += 12 + (long)st.z.size();
  PNGW_REQUIRE(need <= cap, "nbp_png_encode: the file needs %ld bytes, cap is %ld", need, cap);

  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  uint8_t ihdr[13];
  put32(ihdr, (uint32_t)W);
  put32(ihdr + 4, (uint32_t)H);
  ihdr[8] = 8;                  // bit depth
  ihdr[9] = C == 3 ? 2 : 0;     // colour type: truecolour / greyscale
  ihdr[10] = ihdr[11] = ihdr[12] = 0;
  Sink sink{(uint8_t*)out};
  sink.put(sig, 8);
  sink.chunk("IHDR", ihdr, 13, (uint32_t)crc32(crc32(crc32(0, nullptr, 0), (const Bytef*)"IHDR", 4), ihdr, 13));
  for (const Stripe& st : stripes) sink.chunk("IDAT", st.z.data(), (uint32_t)st.z.size(), st.crc);
  sink.chunk("IEND", nullptr, 0, (uint32_t)crc32(crc32(0, nullptr, 0), (const Bytef*)"IEND", 4));
  *len = sink.pos;  // == need
  return 0;
}

}  // extern "C"
