// The JPEG decoder's whole sequence on the CPU, over the decode core the kernels use (dualdiff_amd/csrc/jpeg_decode_core.h):
// unstuffing, the speculative pass, the rounds, verify and repair, the block prefix sum, the output pass, the DC prefix
// sums, the inverse DCT, chroma upsampling and colour conversion — one plain loop where the GPU has one lane.  Every
// buffer is a heap block of exactly the size csrc/jpeg_decode.hip gives it, so that, built with
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/jpeg_decode_host_check.cpp
//
// a read or write outside them, or undefined arithmetic, ends the run.  tests/test_jpeg_input_cpu.py builds and runs it
// over good streams (the pixels must equal the expected ones, at the default rounds and at 0) and over broken ones (the
// run must stay clean and the status must be non-zero).
//
// What this run does NOT cover: only jpeg_decode_core.h is shared with the kernels.  Unstuffing and verify / repair are
// written here as plain sequential loops, so the kernels' own indexing around the core — the count / compact pair of
// dd_jpegd_unstuff_kernel, and dd_jpegd_repair_kernel's ballot, shuffles and carry across groups of 64 entries — is held by
// the GPU equality tests (tests/test_jpeg_input_gpu.py: rounds 0 / 1, guard bytes, byte offsets), not by the sanitizers.
//
// usage: jpeg_decode_host_check CASES    CASES: int32 'DDHC', int32 count, then per case
//   int32 h, w, sampling, rounds (-1: the default), scan_len, lead, want_status (0: zero, 1: non-zero), has_pixels
//   uint8 tables[4016], uint8 scan[lead + scan_len], uint8 pixels[h * w * 3] if has_pixels
// Prints one line per case; exit status 1 if any case misses what it wants.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dualdiff_hip.h"
#include "../dualdiff_amd/csrc/jpeg_decode_core.h"

namespace {

constexpr int kSub = DD_JD_SUB_BITS;

// a heap block of exactly n elements (never empty), zeroed
template <typename T>
struct Block {
  T* p;
  size_t n;
  explicit Block(size_t count) : p(static_cast<T*>(calloc(count ? count : 1, sizeof(T)))), n(count) {
    if (!p) abort();
  }
  ~Block() { free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct Case {
  int32_t h, w, sampling, rounds, scan_len, lead, want_status, has_pixels;
};

// -> status; pixels into out (h * w * 3); *repaired: subsequences the repair pass decoded again
int32_t decode(const Case& c, const DdJdTables* tab, const uint8_t* scan, uint8_t* out, int* repaired, int* nsub_out) {
  const int mcu = c.sampling == 420 ? 16 : 8, bpm = c.sampling == 420 ? 6 : 3;
  const int mw = (c.w + mcu - 1) / mcu, mh = (c.h + mcu - 1) / mcu, nmcu = mw * mh, nblk = nmcu * bpm;
  const int yw = mw * mcu, yh = mh * mcu, cw = mw * 8, ch = mh * 8;
  const int tcw = c.sampling == 420 ? (c.w + 1) / 2 : c.w, tch = c.sampling == 420 ? (c.h + 1) / 2 : c.h;
  const int64_t cap = c.scan_len > 0 ? c.scan_len : 1;
  const int32_t nwords = (int32_t)(up16(cap + 8) / 4);
  const int32_t nsub_cap = (int32_t)((cap * 8 + kSub - 1) / kSub);
  int32_t status = 0;

  // unstuff
  Block<uint32_t> stream((size_t)nwords);
  uint8_t* dst = reinterpret_cast<uint8_t*>(stream.p);
  int64_t at = 0;
  for (int64_t i = 0; i < c.scan_len; ++i) {
    if (scan[i] == 0 && i > 0 && scan[i - 1] == 0xFF) continue;
    dst[at++] = scan[i];
  }
  const int32_t nbits = (int32_t)(at * 8);
  int32_t nsub = (int32_t)(((int64_t)nbits + kSub - 1) / kSub);
  if (nsub > nsub_cap) nsub = nsub_cap;
  *nsub_out = nsub;

  // speculative pass and rounds
  Block<DdJdState> ent((size_t)nsub_cap), ex0((size_t)nsub_cap), ex1((size_t)nsub_cap);
  DdJdState* ex[2] = {ex0.p, ex1.p};
  uint32_t ignored = 0;
  for (int32_t i = 0; i < nsub; ++i) {
    ent.p[i] = DdJdState{i * kSub, 0, 0, 0};
    ex[0][i] = dd_jd_decode_sub<false>(stream.p, nwords, nbits, (i + 1) * kSub, ent.p[i], tab, bpm, nullptr, 0, 0, &ignored);
  }
  int cur = 0;
  const int rounds = c.rounds < 0 ? DD_JPEG_DECODE_ROUNDS : c.rounds;
  for (int r = 0; r < rounds; ++r) {
    for (int32_t i = 0; i < nsub; ++i) {
      const DdJdState e = i ? ex[cur][i - 1] : DdJdState{0, 0, 0, 0};
      if (dd_jd_same(ent.p[i], e)) {
        ex[cur ^ 1][i] = ex[cur][i];
        continue;
      }
      ent.p[i] = e;
      ex[cur ^ 1][i] = dd_jd_decode_sub<false>(stream.p, nwords, nbits, (i + 1) * kSub, e, tab, bpm, nullptr, 0, 0, &ignored);
    }
    cur ^= 1;
  }

  // verify and repair: entry 0 is true; entry i is true if it equals exit i - 1 and entry i - 1 is true
  DdJdState prev = {0, 0, 0, 0};
  *repaired = 0;
  for (int32_t i = 0; i < nsub; ++i) {
    if (!dd_jd_same(ent.p[i], prev)) {
      ent.p[i] = prev;
      ent.p[i].nblk = 0;
      ex[cur][i] = dd_jd_decode_sub<false>(stream.p, nwords, nbits, (i + 1) * kSub, ent.p[i], tab, bpm, nullptr, 0, 0, &ignored);
      ++*repaired;
    }
    prev = ex[cur][i];
  }

  // first block of every subsequence
  Block<int32_t> first((size_t)nsub_cap);
  uint32_t total = 0;
  for (int32_t i = 0; i < nsub; ++i) {
    first.p[i] = (int32_t)(total < (uint32_t)nblk ? total : (uint32_t)nblk);
    total += (uint32_t)(ex[cur][i].nblk > 0 ? ex[cur][i].nblk : 0);
  }
  if (total < (uint32_t)nblk) status |= DD_JD_EXHAUSTED;

  // output pass
  Block<int16_t> coef((size_t)nblk * 64);
  for (int32_t i = 0; i < nsub; ++i) {
    uint32_t flags = 0;
    dd_jd_decode_sub<true>(stream.p, nwords, nbits, (i + 1) * kSub, ent.p[i], tab, bpm, coef.p, first.p[i], nblk, &flags);
    status |= (int32_t)flags;
  }

  // DC differences -> DC values, per component
  for (int comp = 0; comp < 3; ++comp) {
    const int n = nmcu * ((bpm == 6 && comp == 0) ? 4 : 1);
    uint32_t sum = 0;
    for (int j = 0; j < n; ++j) {
      const int b = bpm == 3 ? j * 3 + comp : (comp == 0 ? (j >> 2) * 6 + (j & 3) : j * 6 + 3 + comp);
      sum += (uint32_t)(int32_t)coef.p[(size_t)b * 64];
      coef.p[(size_t)b * 64] = (int16_t)(uint16_t)sum;
    }
  }

  // inverse DCT into the padded planes
  const int64_t c_off = up16((int64_t)yw * yh), c_size = up16((int64_t)cw * ch);
  Block<uint8_t> planes((size_t)(c_off + 2 * c_size));
  for (int32_t b = 0; b < nblk; ++b) {
    const int32_t m = b / bpm, k = b - m * bpm, comp = dd_jd_component(k, bpm);
    const int32_t my = m / mw, mx = m - my * mw;
    int32_t ws[64];
    for (int col = 0; col < 8; ++col) dd_jd_idct_column(coef.p + (size_t)b * 64, tab->q[comp], col, ws);
    for (int row = 0; row < 8; ++row) {
      int64_t where;
      if (comp == 0 && bpm == 6) where = (int64_t)((2 * my + (k >> 1)) * 8 + row) * yw + (2 * mx + (k & 1)) * 8;
      else if (comp == 0) where = (int64_t)(my * 8 + row) * yw + mx * 8;
      else where = c_off + (comp - 1) * c_size + (int64_t)(my * 8 + row) * cw + mx * 8;
      dd_jd_idct_row(ws, row, planes.p + where);
    }
  }

  // upsampling and colour
  const uint8_t* pcb = planes.p + c_off;
  const uint8_t* pcr = pcb + c_size;
  for (int32_t y = 0; y < c.h; ++y)
    for (int32_t x = 0; x < c.w; ++x) {
      int32_t cb, cr;
      if (bpm == 6) {
        cb = dd_jd_upsample(pcb, cw, tch, tcw, y, x);
        cr = dd_jd_upsample(pcr, cw, tch, tcw, y, x);
      } else {
        cb = pcb[(int64_t)y * cw + x];
        cr = pcr[(int64_t)y * cw + x];
      }
      dd_jd_rgb(planes.p[(int64_t)y * yw + x], cb, cr, out + ((int64_t)y * c.w + x) * 3);
    }
  return status;
}

bool take(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CASES\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int32_t head[2];
  if (!take(f, head, sizeof head) || head[0] != 0x43484444 || head[1] < 0) {               // "DDHC" little-endian
    fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 2;
  }
  int failed = 0;
  for (int32_t n = 0; n < head[1]; ++n) {
    Case c;
    if (!take(f, &c, sizeof c) || c.h <= 0 || c.w <= 0 || c.h > 65535 || c.w > 65535 || c.scan_len < 0 || c.lead < 0 ||
        (c.sampling != 420 && c.sampling != 444)) {
      fprintf(stderr, "case %d: bad header\n", n);
      return 2;
    }
    Block<uint8_t> tables(sizeof(DdJdTables)), scan((size_t)c.lead + (size_t)c.scan_len);
    Block<uint8_t> want(c.has_pixels ? (size_t)c.h * c.w * 3 : 0), got((size_t)c.h * c.w * 3);
    if (!take(f, tables.p, tables.n) || !take(f, scan.p, scan.n) || !take(f, want.p, want.n)) {
      fprintf(stderr, "case %d: cut short\n", n);
      return 2;
    }
    DdJdTables tab;
    memcpy(&tab, tables.p, sizeof tab);
    // the segment in a block of its own, so that a read in front of or behind it is caught
    Block<uint8_t> seg((size_t)c.scan_len);
    if (c.scan_len) memcpy(seg.p, scan.p + c.lead, (size_t)c.scan_len);
    int repaired = 0, nsub = 0;
    const int32_t status = decode(c, &tab, seg.p, got.p, &repaired, &nsub);
    size_t differ = 0;
    if (c.has_pixels)
      for (size_t i = 0; i < got.n; ++i) differ += got.p[i] != want.p[i];
    const bool ok = (c.want_status ? status != 0 : status == 0) && differ == 0;
    printf("case %d: %d x %d sampling %d rounds %d scan %d bytes: status %d, %d of %d subsequences repaired, %zu bytes differ%s\n",
           n, c.h, c.w, c.sampling, c.rounds, c.scan_len, status, repaired, nsub, differ, ok ? "" : "  FAILED");
    failed += !ok;
  }
  fclose(f);
  printf("%d cases, %d failed\n", head[1], failed);
  return failed ? 1 : 0;
}
