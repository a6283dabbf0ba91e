// The JPEG decoder's host half and the guards of cft_jpeg_decode_u8 under a host sanitizer, no GPU needed.  The two host functions
// (cft_jpeg_info, cft_jpeg_entropy) are fed a small baseline file - built below: 16 x 16, three components at 4:2:0, a restart
// interval of one MCU, the standard Huffman tables - whole, cut at every byte offset, with a few thousand seeded byte corruptions,
// and bytes that are no JPEG; the coefficient and table buffers are heap blocks of exactly the reported sizes, so a byte written past
// them or read past nbytes stops the program.  The table guards must return CFT_EINVAL before any device call.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/jpeg_guards.hip multispectral-object-detection_amd/csrc/jpeg.hip \
//         multispectral-object-detection_amd/csrc/runtime.hip -o tools/micro/jpeg_guards && tools/micro/jpeg_guards
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include "cft_hip.h"

static int failures = 0;
#define CHECK(cond, what)                                               \
  do {                                                                  \
    if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; }        \
  } while (0)
#define EXPECT_EINVAL(call, what)                                                           \
  do {                                                                                      \
    const int st = (call);                                                                  \
    if (st != CFT_EINVAL) { std::printf("FAIL %s: status %d\n", what, st); ++failures; }    \
    else std::printf("ok   %-40s %s\n", what, cft_last_error());                            \
  } while (0)

typedef std::vector<unsigned char> Bytes;

// ---- a tiny baseline encoder: quantised coefficients in, file bytes out (the standard tables of ITU T.81 annex K)
static const unsigned char DC_L_COUNTS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const unsigned char DC_C_COUNTS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char AC_L_COUNTS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const unsigned char AC_L_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const unsigned char ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Code { unsigned short code[256]; unsigned char len[256]; };
static Code make_code(const unsigned char* counts, const unsigned char* vals) {
  Code c;
  std::memset(&c, 0, sizeof c);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) { c.code[vals[k]] = (unsigned short)code; c.len[vals[k]] = (unsigned char)len; }
    code <<= 1;
  }
  return c;
}

struct Writer {
  Bytes out;
  unsigned acc = 0;
  int nbits = 0;
  void put(unsigned v, int n) {
    for (int i = n - 1; i >= 0; --i) {
      acc = (acc << 1) | ((v >> i) & 1u);
      if (++nbits == 8) { out.push_back((unsigned char)acc); if (acc == 0xFF) out.push_back(0); acc = 0; nbits = 0; }
    }
  }
  void flush() { while (nbits) put(1, 1); }
  void marker(int m) { flush(); out.push_back(0xFF); out.push_back((unsigned char)m); }
  void segment(int m, const Bytes& body) {
    marker(m);
    out.push_back((unsigned char)((body.size() + 2) >> 8)); out.push_back((unsigned char)((body.size() + 2) & 255));
    out.insert(out.end(), body.begin(), body.end());
  }
};

static void put_value(Writer& w, int v, int s) { w.put((unsigned)(v < 0 ? v + (1 << s) - 1 : v), s); }
static int category(int v) { int a = v < 0 ? -v : v, s = 0; while (a) { ++s; a >>= 1; } return s; }

static void put_block(Writer& w, const short* blk, int& pred, const Code& dc, const Code& ac) {
  const int diff = blk[0] - pred;
  pred = blk[0];
  int s = category(diff);
  w.put(dc.code[s], dc.len[s]);
  if (s) put_value(w, diff, s);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[ZIGZAG[k]];
    if (!v) { ++run; continue; }
    while (run > 15) { w.put(ac.code[0xF0], ac.len[0xF0]); run -= 16; }
    s = category(v);
    w.put(ac.code[(run << 4) | s], ac.len[(run << 4) | s]);
    put_value(w, v, s);
    run = 0;
  }
  if (run) w.put(ac.code[0], ac.len[0]);
}

// 16 x 16, Y 2x2 + Cb + Cr, one MCU, restart interval 1 when `wide` (then 32 x 16: two MCUs with a restart marker between them)
static Bytes make_file(const std::vector<short>& coef, bool wide) {
  Writer w;
  w.out = {0xFF, 0xD8};
  w.segment(0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  Bytes q(1, 0);
  for (int i = 0; i < 64; ++i) q.push_back((unsigned char)(1 + (i & 7)));
  w.segment(0xDB, q);
  const int W = wide ? 32 : 16;
  w.segment(0xC0, {8, 0, 16, 0, (unsigned char)W, 3, 1, 0x22, 0, 2, 0x11, 0, 3, 0x11, 0});
  auto dht = [&](int id, const unsigned char* counts, const unsigned char* vals, int n) {
    Bytes b(1, (unsigned char)id);
    b.insert(b.end(), counts, counts + 16);
    b.insert(b.end(), vals, vals + n);
    w.segment(0xC4, b);
  };
  dht(0x00, DC_L_COUNTS, DC_VALS, 12);
  dht(0x10, AC_L_COUNTS, AC_L_VALS, 162);
  dht(0x01, DC_C_COUNTS, DC_VALS, 12);
  if (wide) w.segment(0xDD, {0, 1});
  w.segment(0xDA, {3, 1, 0x00, 2, 0x10, 3, 0x10, 0, 63, 0});
  const Code dcl = make_code(DC_L_COUNTS, DC_VALS), dcc = make_code(DC_C_COUNTS, DC_VALS), acl = make_code(AC_L_COUNTS, AC_L_VALS);
  const int mcus = wide ? 2 : 1, bw = 2 * mcus;
  const long cb0 = 64L * bw * 2, cr0 = cb0 + 64L * mcus;
  int pred[3] = {0, 0, 0};
  for (int m = 0; m < mcus; ++m) {
    if (m) { w.marker(0xD0 + ((m - 1) & 7)); pred[0] = pred[1] = pred[2] = 0; }
    for (int by = 0; by < 2; ++by)
      for (int bx = 0; bx < 2; ++bx) put_block(w, coef.data() + 64L * (by * bw + 2 * m + bx), pred[0], dcl, acl);
    put_block(w, coef.data() + cb0 + 64L * m, pred[1], dcc, acl);
    put_block(w, coef.data() + cr0 + 64L * m, pred[2], dcc, acl);
  }
  w.marker(0xD9);
  return w.out;
}

// info + entropy into heap blocks of exactly the reported sizes; returns the status of the last call made
static int decode(const Bytes& f, long nbytes, std::vector<short>* coef_out = nullptr) {
  // an exact-size copy: a read past nbytes is a heap overflow the sanitizer sees
  unsigned char* bytes = (unsigned char*)std::malloc((size_t)(nbytes > 0 ? nbytes : 1));
  std::memcpy(bytes, f.data(), (size_t)nbytes);
  cft_jpeg_info_t info;
  int st = cft_jpeg_info(bytes, nbytes, &info);
  if (st == CFT_OK) {
    short* coef = (short*)std::malloc((size_t)info.ncoef * sizeof(short));
    unsigned short* qtab = (unsigned short*)std::malloc(CFT_JPEG_QTAB_BYTES);
    st = cft_jpeg_entropy(bytes, nbytes, coef, qtab, &info);
    if (st == CFT_OK && coef_out) coef_out->assign(coef, coef + info.ncoef);
    std::free(coef); std::free(qtab);
  }
  std::free(bytes);
  return st;
}

alignas(16) static unsigned char fake[4096];     // never dereferenced: every table call fails before the launch

static cft_jpeg_desc_t good_row(long plane_off) {
  cft_jpeg_desc_t d;
  std::memset(&d, 0, sizeof d);
  d.coef = (const short*)fake; d.qtab = (const unsigned short*)(fake + 64); d.dst = fake + 128;
  d.width = 33; d.height = 17; d.dst_stride = 99; d.plane_off = plane_off;
  d.ncomp = 3; d.hmax = 2; d.vmax = 2;
  d.bw[0] = 6; d.bh[0] = 4; d.bw[1] = d.bw[2] = 3; d.bh[1] = d.bh[2] = 2;        // 36 blocks: 2304 bytes of planes
  return d;
}

int main() {
  // ---- the host half
  unsigned seed = 12345;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  for (int wide = 0; wide < 2; ++wide) {
    const int blocks = wide ? 12 : 6;
    std::vector<short> coef(64 * blocks, 0);
    for (int b = 0; b < blocks; ++b) {
      coef[64 * b] = (short)((int)(rnd() % 400) - 200);
      for (int k = 1; k < 64; ++k)
        if (rnd() % 5 == 0) coef[64 * b + k] = (short)((int)(rnd() % 61) - 30);
      if (b == 1) { coef[64 * b + 63] = -1; for (int k = 20; k < 63; ++k) coef[64 * b + k] = 0; }      // a run above 16 zeros
    }
    const Bytes file = make_file(coef, wide != 0);
    std::vector<short> back;
    CHECK(decode(file, (long)file.size(), &back) == CFT_OK && back == coef, "the whole file decodes to the coefficients it was written from");
    int ok = 0, unsupported = 0;
    for (long cut = 0; cut < (long)file.size(); ++cut) {
      const int st = decode(file, cut);
      CHECK(st == CFT_JPEG_UNSUPPORTED || st == CFT_EINVAL, "a cut file is refused");
      (st == CFT_JPEG_UNSUPPORTED ? unsupported : ok) += 1;
    }
    std::printf("ok   %s: %ld cuts, %d unsupported, %d einval (the empty one)\n", wide ? "32x16 with restarts" : "16x16", (long)file.size(), unsupported, ok);
    int n_ok = 0, n_bad = 0;
    for (int t = 0; t < 4000; ++t) {
      Bytes f = file;
      const int hits = 1 + (int)(rnd() % 3);
      for (int h = 0; h < hits; ++h) f[rnd() % f.size()] = (unsigned char)rnd();
      const int st = decode(f, (long)f.size());
      CHECK(st == CFT_OK || st == CFT_JPEG_UNSUPPORTED, "a corrupted file decodes or is refused");
      (st == CFT_OK ? n_ok : n_bad) += 1;
    }
    std::printf("ok   4000 corruptions: %d still decode, %d refused\n", n_ok, n_bad);
  }
  {
    Bytes junk(3000);
    for (auto& b : junk) b = (unsigned char)rnd();
    CHECK(decode(junk, (long)junk.size()) == CFT_JPEG_UNSUPPORTED, "random bytes");
    const Bytes png = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 0x0D, 'I', 'H', 'D', 'R'};
    CHECK(decode(png, (long)png.size()) == CFT_JPEG_UNSUPPORTED, "PNG bytes");
    Bytes ff(500, 0xFF);
    ff[1] = 0xD8;
    CHECK(decode(ff, (long)ff.size()) == CFT_JPEG_UNSUPPORTED, "SOI and fill bytes only");
    cft_jpeg_info_t info;
    CHECK(cft_jpeg_info(nullptr, 10, &info) == CFT_EINVAL && cft_jpeg_info(png.data(), 10, nullptr) == CFT_EINVAL && cft_jpeg_info(png.data(), 0, &info) == CFT_EINVAL,
          "null pointers and empty input");
  }

  // ---- the table guards of cft_jpeg_decode_u8: two rows, the second carries the fault
  unsigned char* dev = fake + 1024;
  const long ws_bytes = 8192;
  auto run = [&](const std::function<void(cft_jpeg_desc_t&)>& spoil) {
    std::vector<cft_jpeg_desc_t> rows = {good_row(0), good_row(2304)};
    spoil(rows[1]);
    return cft_jpeg_decode_u8(dev, rows.data(), 2, fake + 2048, ws_bytes, nullptr);
  };
  std::vector<cft_jpeg_desc_t> rows = {good_row(0), good_row(2304)};
  EXPECT_EINVAL(cft_jpeg_decode_u8(nullptr, rows.data(), 2, fake, ws_bytes, nullptr), "null device table");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, nullptr, 2, fake, ws_bytes, nullptr), "null host table");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, rows.data(), 2, nullptr, ws_bytes, nullptr), "null workspace");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev + 4, rows.data(), 2, fake, ws_bytes, nullptr), "misaligned device table");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, rows.data(), 2, fake + 8, ws_bytes, nullptr), "misaligned workspace");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, rows.data(), 0, fake, ws_bytes, nullptr), "n = 0");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, rows.data(), 65536, fake, ws_bytes, nullptr), "n above the grid limit");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, rows.data(), 2, fake, 0, nullptr), "empty workspace");
  EXPECT_EINVAL(cft_jpeg_decode_u8(dev, rows.data(), 2, fake, 4607, nullptr), "workspace one byte short");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.coef = nullptr; }), "null coefficients");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.qtab = nullptr; }), "null tables");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.dst = nullptr; }), "null destination");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.coef = (const short*)(fake + 1); }), "misaligned coefficients");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.qtab = (const unsigned short*)(fake + 65); }), "misaligned tables");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.width = 0; }), "width = 0");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.height = -3; }), "negative height");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.width = 16385; d.dst_stride = 3L * 16385; }), "width above the size limit");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.ncomp = 2; }), "two components");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.ncomp = 4; }), "four components");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.hmax = 1; d.vmax = 2; }), "luma sampled 1x2");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.hmax = 4; }), "luma sampled 4x2");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.hmax = 0; }), "luma sampling 0");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.ncomp = 1; }), "one component sampled 2x2");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.bw[0] = 5; }), "a block grid too narrow");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.bh[2] = 1 << 20; }), "a block grid far too tall");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.hmax = d.vmax = 1; }), "the block grid of another sampling");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.dst_stride = 98; }), "short row stride");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.dst_stride = -99; }), "negative row stride");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.plane_off = 2308; }), "plane offset not a multiple of 16");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.plane_off = -16; }), "negative plane offset");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.plane_off = 2288; }), "planes overlap the previous row's");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.plane_off = 0; }), "planes at the previous row's offset");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.plane_off = 8192 - 2304 + 16; }), "planes beyond the workspace");
  EXPECT_EINVAL(run([](cft_jpeg_desc_t& d) { d.plane_off = 1L << 40; }), "plane offset far beyond the workspace");

  // the good table itself passes every guard: it would launch, which this program must not do - so it is not called
  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("all guards hold\n");
  return 0;
}
