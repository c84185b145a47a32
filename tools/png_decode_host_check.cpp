// The PNG decoder's whole sequence on the CPU, over the decode core the kernels use (dualdiff_amd/csrc/png_decode_core.h):
// the zlib header, the walk over the blocks, the trailer, the per-chunk decode with its verification, the Adler-32 from
// 16 KiB segments, the unfilter and the conversion — one plain loop where the GPU has a wave.  Every buffer is a heap block
// of exactly the size the format gives it, so that, built with
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/png_decode_host_check.cpp
//
// a read or write outside them, or undefined arithmetic, ends the run.  tests/test_png_input_cpu.py builds and runs it over
// good files (the pixels must equal the constructed ones) and over broken ones (the run must stay clean and the status
// must be the one the breakage names).
//
// What this run does NOT cover: only png_decode_core.h is shared with the kernels.  The window in LDS, its flushes to global
// memory, the wave's match copy and the skewed unfilter schedule of csrc/png_decode.hip are held by the GPU equality tests
// (tests/test_png_input_gpu.py), not by the sanitizers.
//
// usage: png_decode_host_check FILE.png ...
// Per file one line: `FILE h w colour status chunked`, chunked 1 when every chunk of a file of dd_png_encode_u8's shape
// verified (its result is then compared with the sequential one: a difference is `MISMATCH` and exit status 1).  With
// status 0 the RGB pixels go to FILE.rgb.  The chunk framing is walked without CRC checks (pipeline/png_input.py has them).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dualdiff_hip.h"
#include "../dualdiff_amd/csrc/png_decode_core.h"

namespace {

constexpr int64_t kSeg = 16384;

// a heap block of exactly n bytes (never empty), zeroed
struct Block {
  uint8_t* p;
  size_t n;
  explicit Block(size_t count) : p(static_cast<uint8_t*>(calloc(count ? count : 1, 1))), n(count) {
    if (!p) abort();
  }
  ~Block() { free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

// where the host's inflate goes: out[0, limit), one caller
struct HostCtx {
  uint8_t* out;
  bool leader() const { return true; }
  void sync() const {}
  void lit(uint32_t pos, uint32_t byte) { out[pos] = (uint8_t)byte; }
  void copy(uint32_t pos, uint32_t len, uint32_t dist) {
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i % dist];
  }
  void stored(const uint8_t* src, uint32_t pos, uint32_t n) { memcpy(out + pos, src, n); }
  void advance(uint32_t) {}
};

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// the stream kernel's sequence: -> status; filt[0, len) and *adler on success
uint32_t sequential(const uint8_t* s, int64_t n, uint8_t* filt, uint32_t len, uint32_t* adler) {
  DdPdBits br;
  dd_pd_open(br, s, n);
  const uint32_t cmf = dd_pd_take(br, 8), flg = dd_pd_take(br, 8);
  if (dd_pd_over(br)) return DD_PD_TRUNCATED;
  if (!dd_pd_zlib_header_ok(cmf, flg)) return DD_PD_BAD_ZLIB;
  Block shared(sizeof(DdPdShared));
  DdPdShared* sh = reinterpret_cast<DdPdShared*>(shared.p);
  HostCtx ctx = {filt};
  uint32_t pos = 0;
  int final_seen = 0;
  uint32_t err = dd_pd_inflate(br, sh, ctx, len, -1, &pos, &final_seen);
  if (!err && pos < len) err = DD_PD_TOO_SHORT;
  if (!err) err = dd_pd_trailer(br, adler);
  return err;
}

// the chunk kernel's sequence for every chunk: true if all of them verify
bool chunks(const uint8_t* s, int64_t n, const std::vector<int64_t>& tab, uint8_t* filt, uint32_t len) {
  const int nchunk = (int)tab.size() - 1;
  bool all = true;
  for (int c = 0; c < nchunk; ++c) {
    const bool last = c == nchunk - 1;
    const int64_t t0 = tab[c], t1 = tab[c + 1], lo = t0 + (c == 0 ? 2 : 0), hi = t1 - (last ? 4 : 0);
    const uint32_t want = (uint32_t)((int64_t)len - c * kSeg < kSeg ? (int64_t)len - c * kSeg : kSeg);
    bool ok = t0 >= 0 && t1 <= n && lo <= hi;
    if (ok) {
      Block payload((size_t)(hi - lo));                      // its own block: a read past the payload is a finding
      memcpy(payload.p, s + lo, (size_t)(hi - lo));
      Block slot(want);
      Block shared(sizeof(DdPdShared));
      DdPdBits br;
      dd_pd_open(br, payload.p, hi - lo);
      HostCtx ctx = {slot.p};
      uint32_t pos = 0;
      int final_seen = 0;
      const uint32_t err = dd_pd_inflate(br, reinterpret_cast<DdPdShared*>(shared.p), ctx, want, (hi - lo) * 8, &pos, &final_seen);
      ok = err == 0 && pos == want && br.used == (hi - lo) * 8 && (final_seen != 0) == last;
      if (ok) memcpy(filt + c * kSeg, slot.p, want);
    }
    all = all && ok;
  }
  return all;
}

uint32_t adler_of(const uint8_t* filt, uint32_t len) {
  uint32_t A = 1, B = 0;
  for (int64_t at = 0; at < len; at += kSeg) {
    const int64_t n = len - at < kSeg ? len - at : kSeg;
    uint32_t a, b;
    dd_pd_adler_sums(filt + at, n, &a, &b);
    dd_pd_adler_join(&A, &B, a, b, n);
  }
  return (B << 16) | A;
}

// -> status; rgb[h * w * 3]
uint32_t unfilter(uint8_t* filt, int h, int w, int bpp, uint8_t* rgb) {
  const int64_t row = 1 + (int64_t)bpp * w;
  uint32_t bad = 0;
  for (int y = 0; y < h; ++y) {
    uint8_t* cur = filt + y * row;
    int type = cur[0];
    if (type > 4) {
      bad = DD_PD_BAD_FILTER;
      type = 0;
    }
    for (int64_t k = 0; k < row - 1; ++k) {
      const uint32_t a = k >= bpp ? cur[1 + k - bpp] : 0u, b = y > 0 ? cur[1 + k - row] : 0u;
      const uint32_t c = (k >= bpp && y > 0) ? cur[1 + k - bpp - row] : 0u;
      cur[1 + k] = (uint8_t)dd_pd_unfilter(type, cur[1 + k], a, b, c);
    }
    for (int x = 0; x < w; ++x)
      for (int ch = 0; ch < 3; ++ch) rgb[((int64_t)y * w + x) * 3 + ch] = cur[1 + (int64_t)x * bpp + (bpp == 1 ? 0 : ch)];
  }
  return bad;
}

int run(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    printf("%s: cannot open\n", path);
    return 1;
  }
  std::vector<uint8_t> data;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
  fclose(f);
  if (data.size() < 8 + 25 || memcmp(data.data(), "\x89PNG\r\n\x1a\n", 8) != 0) {
    printf("%s: not a PNG\n", path);
    return 1;
  }
  const int w = (int)be32(&data[16]), h = (int)be32(&data[20]), colour = data[25];
  const int bpp = dd_pd_bpp(colour);
  if (data[24] != 8 || !bpp || w <= 0 || h <= 0 || (int64_t)h * (1 + 4 * (int64_t)w) > (1 << 28)) {
    printf("%s: not built\n", path);
    return 1;
  }
  std::vector<uint8_t> stream;
  std::vector<int64_t> tab(1, 0);
  for (size_t pos = 8; pos + 12 <= data.size();) {
    const size_t length = be32(&data[pos]);
    if (pos + 12 + length > data.size()) break;
    if (memcmp(&data[pos + 4], "IDAT", 4) == 0) {
      stream.insert(stream.end(), data.begin() + pos + 8, data.begin() + pos + 8 + length);
      tab.push_back((int64_t)stream.size());
    }
    pos += 12 + length;
  }
  const uint32_t len = (uint32_t)h * (1u + (uint32_t)bpp * (uint32_t)w);
  Block s(stream.size());                                    // exactly the stream: a read past it is a finding
  memcpy(s.p, stream.data(), stream.size());
  Block filt(len), rgb((size_t)h * w * 3);
  uint32_t adler = 0;
  uint32_t status = sequential(s.p, (int64_t)s.n, filt.p, len, &adler);
  int chunked = 0;
  const int64_t want = ((int64_t)len + kSeg - 1) / kSeg;
  if (colour == 2 && (int64_t)tab.size() - 1 == want) {
    Block again(len);
    if (chunks(s.p, (int64_t)s.n, tab, again.p, len)) {
      chunked = 1;
      if (status != 0 || memcmp(again.p, filt.p, len) != 0) {
        printf("%s MISMATCH: every chunk verifies, the sequential decode has status %u or other bytes\n", path, status);
        return 1;
      }
    }
  }
  if (!status && adler_of(filt.p, len) != adler) status = DD_PD_BAD_ADLER;
  if (!status) status = unfilter(filt.p, h, w, bpp, rgb.p);
  printf("%s %d %d %d %u %d\n", path, h, w, colour, status, chunked);
  if (!status) {
    const std::string out = std::string(path) + ".rgb";
    FILE* o = fopen(out.c_str(), "wb");
    if (!o || fwrite(rgb.p, 1, rgb.n, o) != rgb.n) {
      printf("%s: cannot write\n", out.c_str());
      return 1;
    }
    fclose(o);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(DD_PNG_TRUNCATED == DD_PD_TRUNCATED && DD_PNG_BAD_BLOCK == DD_PD_BAD_BLOCK && DD_PNG_BAD_STORED == DD_PD_BAD_STORED &&
                DD_PNG_BAD_LENGTHS == DD_PD_BAD_LENGTHS && DD_PNG_BAD_SYMBOL == DD_PD_BAD_SYMBOL &&
                DD_PNG_BAD_DISTANCE == DD_PD_BAD_DISTANCE && DD_PNG_TOO_LONG == DD_PD_TOO_LONG &&
                DD_PNG_TOO_SHORT == DD_PD_TOO_SHORT && DD_PNG_BAD_ADLER == DD_PD_BAD_ADLER && DD_PNG_BAD_ZLIB == DD_PD_BAD_ZLIB &&
                DD_PNG_BAD_FILTER == DD_PD_BAD_FILTER, "the header's status bits are the core's");
  int failed = 0;
  for (int i = 1; i < argc; ++i) failed += run(argv[i]);
  printf("%d files, %d failed\n", argc - 1, failed);
  return failed ? 1 : 0;
}
