// The JPEG encoder's host half and the guards of cft_jpeg_encode_coef under a host sanitizer, no GPU needed.  The host functions
// (cft_jpeg_layout, cft_jpeg_quality_tables, cft_jpeg_write_bound, cft_jpeg_write) run over the geometries of the test matrix (ten
// sizes, grey / 4:4:4 / 4:2:2 / 4:2:0) with seeded coefficients, into heap blocks of exactly the stated sizes: the coefficient block
// holds info.ncoef values, the output block `cap` bytes - the bound, the exact file size, and a ladder of shorter capacities down to
// zero - so a byte read or written past either stops the program.  Hostile coefficient buffers (every int16 extreme, garbage in dummy
// blocks) are refused or ignored as the header says.  The table guards must return CFT_EINVAL before any device call.  Build and
// run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/jpeg_encode_guards.hip multispectral-object-detection_amd/csrc/jpeg_encode.hip \
//         multispectral-object-detection_amd/csrc/jpeg.hip multispectral-object-detection_amd/csrc/runtime.hip \
//         -o tools/micro/jpeg_encode_guards && tools/micro/jpeg_encode_guards
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
    else std::printf("ok   %-44s %s\n", what, cft_last_error());                            \
  } while (0)

static unsigned seed = 2468;
static unsigned rnd() { seed = seed * 1664525u + 1013904223u; return seed >> 8; }

// cft_jpeg_write into a heap block of exactly `cap` bytes (at least one is allocated; none of it may be touched when cap is 0)
static int write_into(const short* coef, const unsigned short* qtab, const cft_jpeg_info_t& info, long cap, long* nbytes, std::vector<unsigned char>* keep = nullptr) {
  unsigned char* out = (unsigned char*)std::malloc((size_t)(cap > 0 ? cap : 1));
  const int st = cft_jpeg_write(coef, qtab, &info, out, cap, nbytes);
  if (st == CFT_OK && keep) keep->assign(out, out + *nbytes);
  std::free(out);
  return st;
}

// the file read back by the decoder's host half: the coefficients of the real blocks must be the ones written
static bool reads_back(const std::vector<unsigned char>& file, const cft_jpeg_info_t& info, const short* coef) {
  cft_jpeg_info_t back;
  if (cft_jpeg_info(file.data(), (long)file.size(), &back) != CFT_OK || std::memcmp(&back, &info, sizeof info) != 0) return false;
  short* got = (short*)std::malloc((size_t)info.ncoef * sizeof(short));
  unsigned short qt[192];
  bool same = cft_jpeg_entropy(file.data(), (long)file.size(), got, qt, &back) == CFT_OK;
  long base = 0;
  for (int c = 0; same && c < info.ncomp; ++c) {
    const int rw = (info.cw[c] + 7) / 8, rh = (info.ch[c] + 7) / 8;
    for (int by = 0; by < rh; ++by)
      for (int bx = 0; bx < rw; ++bx)
        if (std::memcmp(got + base + 64L * (by * info.bw[c] + bx), coef + base + 64L * (by * info.bw[c] + bx), 128) != 0) same = false;
    base += 64L * info.bw[c] * info.bh[c];
  }
  std::free(got);
  return same;
}

alignas(16) static unsigned char fake[4096];     // device pointers: never dereferenced, every table call fails before the launch
alignas(16) static unsigned short host_tabs[192];

static cft_jpeg_enc_desc_t good_row() {
  cft_jpeg_enc_desc_t d;
  std::memset(&d, 0, sizeof d);
  d.src = fake; d.qtab = (const unsigned short*)(fake + 512); d.qtab_host = host_tabs; d.coef = (short*)(fake + 1024);
  d.width = 33; d.height = 17; d.src_stride = 99;
  d.ncomp = 3; d.hmax = 2; d.vmax = 2;
  d.bw[0] = 6; d.bh[0] = 4; d.bw[1] = d.bw[2] = 3; d.bh[1] = d.bh[2] = 2;
  return d;
}

int main() {
  // ---- the host half over the matrix's geometries
  const int sizes[10][2] = {{1, 1}, {7, 5}, {8, 8}, {16, 16}, {17, 33}, {40, 24}, {36, 20}, {9, 50}, {41, 3}, {64, 48}};      // width, height
  const int layouts[4][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};
  const int qualities[5] = {90, 92, 95, 98, 100};      // entries <= 24: the decoder's own limit |coef| * q <= 32767 holds for 10-bit values
  int files = 0, short_caps = 0;
  for (int s = 0; s < 10; ++s)
    for (int l = 0; l < 4; ++l) {
      cft_jpeg_info_t info;
      CHECK(cft_jpeg_layout(sizes[s][0], sizes[s][1], layouts[l][0], layouts[l][1], layouts[l][2], &info) == CFT_OK, "layout of a matrix geometry");
      unsigned short qtab[192];
      CHECK(cft_jpeg_quality_tables(qualities[(s + l) % 5], qtab) == CFT_OK, "tables");
      short* coef = (short*)std::malloc((size_t)info.ncoef * sizeof(short));                    // exactly ncoef values
      const bool dense = (s + l) % 3 == 0;
      for (long i = 0; i < info.ncoef; ++i) {
        if (i % 64 == 0) coef[i] = (short)((int)(rnd() % 2001) - 1000);                         // any two differ by at most 11 bits
        else coef[i] = (dense || rnd() % 4 == 0) ? (short)((int)(rnd() % 2047) - 1023) : 0;
      }
      long bound = 0;
      CHECK(cft_jpeg_write_bound(&info, &bound) == CFT_OK && bound > 0, "a bound for a matrix geometry");
      long n = -1;
      std::vector<unsigned char> file;
      CHECK(write_into(coef, qtab, info, bound, &n, &file) == CFT_OK && n > 0 && n <= bound, "a file fits its bound");
      CHECK(reads_back(file, info, coef), "the decoder reads the coefficients back");
      long m = -1;
      CHECK(write_into(coef, qtab, info, n, &m) == CFT_OK && m == n, "the exact size is enough");
      const long caps[] = {n - 1, n - 2, n - 3, n - 5, n / 2, n / 3, 700, 623, 400, 180, 21, 20, 4, 2, 1, 0};
      for (long cap : caps) {
        if (cap < 0 || cap >= n) continue;
        long k = -1;
        CHECK(write_into(coef, qtab, info, cap, &k) == CFT_JPEG_SHORT_BUFFER && k == 0, "a short buffer is reported");
        ++short_caps;
      }
      // hostile buffers: every extreme in turn at a real block's DC and at an AC position
      const short extremes[] = {-32768, 32767, 2048, -2048, 1024, -1024};
      for (short e : extremes) {
        const short dc = coef[0], ac = coef[5];
        long k = -1;
        coef[0] = e;
        const int st_dc = write_into(coef, qtab, info, bound, &k);
        CHECK(((e >= 2048 || e <= -2048) ? st_dc == CFT_JPEG_UNSUPPORTED && k == 0 : st_dc == CFT_OK), "a DC difference beyond 11 bits is refused");
        coef[0] = dc;
        coef[5] = e;                                                                             // block 0 is always real
        CHECK(write_into(coef, qtab, info, bound, &k) == CFT_JPEG_UNSUPPORTED && k == 0, "an AC value beyond 10 bits is refused");
        coef[5] = ac;
      }
      // garbage in the dummy blocks changes no byte
      {
        std::vector<unsigned char> clean, dirty;
        long k = -1;
        CHECK(write_into(coef, qtab, info, bound, &k, &clean) == CFT_OK, "clean");
        const int rw = (info.cw[0] + 7) / 8, rh = (info.ch[0] + 7) / 8;
        int dummies = 0;
        for (int by = 0; by < info.bh[0]; ++by)
          for (int bx = 0; bx < info.bw[0]; ++bx)
            if (by >= rh || bx >= rw) {
              for (int i = 0; i < 64; ++i) coef[64L * (by * info.bw[0] + bx) + i] = (short)(i & 1 ? -32768 : 32767);
              ++dummies;
            }
        CHECK(write_into(coef, qtab, info, bound, &k, &dirty) == CFT_OK && dirty == clean, "dummy blocks are not read");
        if (sizes[s][0] == 36 && l == 3) CHECK(dummies == 9, "36 x 20 at 4:2:0 has a dummy column and a dummy row");
      }
      std::free(coef);
      ++files;
    }
  std::printf("ok   %d geometries written, read back, cut at %d capacities, fed extremes and dummy garbage\n", files, short_caps);

  {
    cft_jpeg_info_t info;
    unsigned short qtab[192];
    long n = 0;
    unsigned char out[64];
    short coef[64] = {0};
    CHECK(cft_jpeg_layout(0, 1, 1, 1, 1, &info) == CFT_EINVAL && cft_jpeg_layout(1, 16385, 1, 1, 1, &info) == CFT_EINVAL &&
          cft_jpeg_layout(8, 8, 2, 1, 1, &info) == CFT_EINVAL && cft_jpeg_layout(8, 8, 3, 1, 2, &info) == CFT_EINVAL &&
          cft_jpeg_layout(8, 8, 1, 2, 2, &info) == CFT_EINVAL && cft_jpeg_layout(8, 8, 3, 1, 1, nullptr) == CFT_EINVAL, "layouts outside the subset");
    CHECK(cft_jpeg_quality_tables(0, qtab) == CFT_EINVAL && cft_jpeg_quality_tables(101, qtab) == CFT_EINVAL && cft_jpeg_quality_tables(50, nullptr) == CFT_EINVAL, "qualities");
    CHECK(cft_jpeg_layout(8, 8, 1, 1, 1, &info) == CFT_OK && cft_jpeg_quality_tables(50, qtab) == CFT_OK, "a good pair");
    CHECK(cft_jpeg_write(nullptr, qtab, &info, out, 64, &n) == CFT_EINVAL && cft_jpeg_write(coef, nullptr, &info, out, 64, &n) == CFT_EINVAL &&
          cft_jpeg_write(coef, qtab, nullptr, out, 64, &n) == CFT_EINVAL && cft_jpeg_write(coef, qtab, &info, nullptr, 64, &n) == CFT_EINVAL &&
          cft_jpeg_write(coef, qtab, &info, out, 64, nullptr) == CFT_EINVAL && cft_jpeg_write(coef, qtab, &info, out, -1, &n) == CFT_EINVAL, "null pointers, negative cap");
    cft_jpeg_info_t bad = info;
    bad.bw[0] = 1 << 20;
    long b1 = 7, b2 = 7;
    CHECK(cft_jpeg_write(coef, qtab, &bad, out, 64, &n) == CFT_EINVAL && cft_jpeg_write_bound(&bad, &b1) == CFT_EINVAL && b1 == -1 &&
          cft_jpeg_write_bound(nullptr, &b2) == CFT_EINVAL && b2 == -1 && cft_jpeg_write_bound(&info, nullptr) == CFT_EINVAL, "an info nobody laid out");
    bad = info;
    bad.ncoef = 1L << 40;
    CHECK(cft_jpeg_write(coef, qtab, &bad, out, 64, &n) == CFT_EINVAL, "an inflated coefficient count");
    qtab[9] = 0;
    CHECK(cft_jpeg_write(coef, qtab, &info, out, 64, &n) == CFT_EINVAL, "a zero table entry");
    qtab[9] = 256;
    CHECK(cft_jpeg_write(coef, qtab, &info, out, 64, &n) == CFT_EINVAL, "a 9-bit table entry");
  }

  // ---- the table guards of cft_jpeg_encode_coef: two rows, the second carries the fault
  for (int i = 0; i < 192; ++i) host_tabs[i] = (unsigned short)(1 + i % 255);
  unsigned char* dev = fake + 2048;
  auto run = [&](const std::function<void(cft_jpeg_enc_desc_t&)>& spoil) {
    std::vector<cft_jpeg_enc_desc_t> rows = {good_row(), good_row()};
    spoil(rows[1]);
    return cft_jpeg_encode_coef(dev, rows.data(), 2, nullptr);
  };
  std::vector<cft_jpeg_enc_desc_t> rows = {good_row(), good_row()};
  static unsigned short zero_tab[192], wide_tab[192], grey_tab[192];
  for (int i = 0; i < 192; ++i) { zero_tab[i] = 3; wide_tab[i] = 3; grey_tab[i] = i < 64 ? 3 : 0; }
  zero_tab[191] = 0; wide_tab[64] = 256;
  EXPECT_EINVAL(cft_jpeg_encode_coef(nullptr, rows.data(), 2, nullptr), "null device table");
  EXPECT_EINVAL(cft_jpeg_encode_coef(dev, nullptr, 2, nullptr), "null host table");
  EXPECT_EINVAL(cft_jpeg_encode_coef(dev + 4, rows.data(), 2, nullptr), "misaligned device table");
  EXPECT_EINVAL(cft_jpeg_encode_coef(dev, (const char*)rows.data() + 4, 1, nullptr), "misaligned host table");
  EXPECT_EINVAL(cft_jpeg_encode_coef(dev, rows.data(), 0, nullptr), "n = 0");
  EXPECT_EINVAL(cft_jpeg_encode_coef(dev, rows.data(), -2, nullptr), "negative n");
  EXPECT_EINVAL(cft_jpeg_encode_coef(dev, rows.data(), 65536, nullptr), "n above the grid limit");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.src = nullptr; }), "null source");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab = nullptr; }), "null device tables");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab_host = nullptr; }), "null host tables");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.coef = nullptr; }), "null coefficients");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.coef = (short*)(fake + 1024 + 8); }), "coefficients not 16-byte aligned");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.coef = (short*)(fake + 1024 + 1); }), "coefficients at an odd address");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab = (const unsigned short*)(fake + 513); }), "misaligned device tables");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab_host = (const unsigned short*)((const char*)host_tabs + 1); }), "misaligned host tables");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.width = 0; }), "width = 0");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.height = -3; }), "negative height");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.width = 16385; d.src_stride = 3L * 16385; }), "width above the size limit");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.height = 1 << 30; }), "height far above the size limit");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.ncomp = 2; }), "two components");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.ncomp = 4; }), "four components");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.ncomp = 0; }), "no components");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.hmax = 1; d.vmax = 2; }), "luma sampled 1x2");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.hmax = 4; }), "luma sampled 4x2");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.hmax = 0; }), "luma sampling 0");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.vmax = -2; }), "negative sampling");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.ncomp = 1; d.qtab_host = grey_tab; }), "one component sampled 2x2");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.bw[0] = 5; }), "a block grid too narrow");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.bh[2] = 1 << 20; }), "a block grid far too tall");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.bw[1] = -3; }), "a negative block grid");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.hmax = d.vmax = 1; }), "the block grid of another sampling");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.ncomp = 1; d.hmax = d.vmax = 1; d.src_stride = 33; d.bw[0] = 5; d.bh[0] = 3; d.qtab_host = grey_tab; }),
                "grey with chroma grids left in the row");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.src_stride = 98; }), "short row stride");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.src_stride = -99; }), "negative row stride");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.src_stride = 0; }), "zero row stride");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab_host = zero_tab; }), "a zero in the last table entry");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab_host = wide_tab; }), "a 9-bit chroma table entry");
  EXPECT_EINVAL(run([](cft_jpeg_enc_desc_t& d) { d.qtab_host = grey_tab; }), "colour with the tables of a grey image");

  // the good table itself passes every guard: it would launch, which this program must not do - so it is not called
  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("all guards hold\n");
  return 0;
}
