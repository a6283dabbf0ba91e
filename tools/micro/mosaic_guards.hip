// Host-side guards of cft_mosaic_compose / _slots / _finish / _area and of the two new flags of cft_detect_render under a host
// sanitizer, no GPU needed: every call below must return CFT_EINVAL from the checks in front of the launch (nothing is launched,
// no HIP call is made).  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/mosaic_guards.hip multispectral-object-detection_amd/csrc/mosaic.hip multispectral-object-detection_amd/csrc/detect.hip \
//         multispectral-object-detection_amd/csrc/runtime.hip -o tools/micro/mosaic_guards && tools/micro/mosaic_guards
#include <cstdio>
#include <cstring>
#include <vector>
#include "cft_hip.h"

static int failures = 0;
#define EXPECT_EINVAL(call, what)                                                           \
  do {                                                                                      \
    const int st = (call);                                                                  \
    if (st != CFT_EINVAL) { std::printf("FAIL %s: status %d\n", what, st); ++failures; }    \
    else std::printf("ok   %-34s %s\n", what, cft_last_error());                            \
  } while (0)

int main() {
  // never dereferenced: every call fails before the launch
  alignas(16) static unsigned char fake[4096 * 64];
  unsigned char* u = fake;
  int* ip = (int*)fake;
  const float* fp = (const float*)fake;
  const double sf = 0.5, bad_sf = 0.0, nan_sf = 0.0 / 0.0;

  // compose: a [5, 6, 75, 100] uint8 batch into a 3 x 3 grid of 48 x 64 cells
  auto compose = [&](const void* img, int dt, int B, int C, int H, int W, int c0, int bs, int ns, int h, int w, int resize, unsigned char* m, long ms, int* key) {
    return cft_mosaic_compose(img, dt, B, C, H, W, 6L * H * W, (long)H * W, W, 1, c0, bs, ns, h, w, resize, m, ms, key, nullptr);
  };
  EXPECT_EINVAL(compose(nullptr, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 3, 48, 64, 1, u, 576, ip), "compose: null images");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 3, 48, 64, 1, u, 576, nullptr), "compose: null maxkey");
  EXPECT_EINVAL(compose(u, 3, 5, 6, 75, 100, 0, 5, 3, 48, 64, 1, u, 576, ip), "compose: unknown dtype");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 4, 5, 3, 48, 64, 1, u, 576, ip), "compose: channels beyond C");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 2, 75, 100, 0, 5, 3, 48, 64, 1, u, 576, ip), "compose: two channels");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 6, 3, 48, 64, 1, u, 576, ip), "compose: bs above B");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 2, 48, 64, 1, u, 576, ip), "compose: ns too small");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 4, 48, 64, 1, u, 768, ip), "compose: ns too large");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 3, 76, 64, 1, u, 576, ip), "compose: cell taller than image");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 3, 48, 64, 0, u, 576, ip), "compose: no resize, other size");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 3, 48, 64, 1, u, 575, ip), "compose: short mosaic stride");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, 0, 5, 3, 48, 64, 1, u, 576, (int*)(fake + 2)), "compose: misaligned maxkey");
  EXPECT_EINVAL(compose(u, CFT_MOSAIC_U8, 300, 6, 32768, 32768, 0, 260, 17, 32768, 32768, 0, u, 1L << 30, ip), "compose: mosaic too large");
  EXPECT_EINVAL(cft_mosaic_compose(u, CFT_MOSAIC_U8, 5, 6, 75, 100, -1, 7500, 100, 1, 0, 5, 3, 48, 64, 1, u, 576, ip, nullptr), "compose: negative stride");

  // slots
  auto rows = [&](const void* r, int nt, int cols, int f64, int bs, int cap, int nc, int h, int w, const double* s, int* out, int* flag) {
    return cft_mosaic_slots(r, nt, cols, f64, nullptr, nullptr, 0, 0, bs, cap, nc, h, w, s, out, flag, nullptr);
  };
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 3, 48, 64, &sf, nullptr, ip), "slots: null slots");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 3, 48, 64, nullptr, ip, ip), "slots: null scale factor");
  EXPECT_EINVAL(rows(nullptr, 10, 6, 0, 5, 8, 3, 48, 64, &sf, ip, ip), "slots: neither rows nor dets");
  EXPECT_EINVAL(cft_mosaic_slots(u, 10, 6, 0, fp, ip, 5, 8, 5, 8, 3, 48, 64, &sf, ip, ip, nullptr), "slots: rows and dets");
  EXPECT_EINVAL(rows(u, 0, 6, 0, 5, 8, 3, 48, 64, &sf, ip, ip), "slots: nt = 0");
  EXPECT_EINVAL(rows(u, 10, 5, 0, 5, 8, 3, 48, 64, &sf, ip, ip), "slots: five columns");
  EXPECT_EINVAL(rows(u + 4, 10, 7, 1, 5, 8, 3, 48, 64, &sf, ip, ip), "slots: misaligned float64 rows");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 0, 8, 3, 48, 64, &sf, ip, ip), "slots: bs = 0");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 0, 3, 48, 64, &sf, ip, ip), "slots: cap = 0");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 1 << 28, 3, 48, 64, &sf, ip, ip), "slots: table too large");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 0, 48, 64, &sf, ip, ip), "slots: nc = 0");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 3, 0, 64, &sf, ip, ip), "slots: h = 0");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 3, 48, 64, &bad_sf, ip, ip), "slots: scale factor 0");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 3, 48, 64, &nan_sf, ip, ip), "slots: scale factor NaN");
  EXPECT_EINVAL(rows(u, 10, 6, 0, 5, 8, 3, 48, 64, &sf, (int*)(fake + 8), ip), "slots: misaligned slots");
  EXPECT_EINVAL(cft_mosaic_slots(nullptr, 0, 0, 0, fp, nullptr, 5, 8, 5, 8, 3, 48, 64, &sf, ip, ip, nullptr), "slots: dets without counts");
  EXPECT_EINVAL(cft_mosaic_slots(nullptr, 0, 0, 0, fp, ip, 4, 8, 5, 8, 3, 48, 64, &sf, ip, ip, nullptr), "slots: bs above B");
  EXPECT_EINVAL(cft_mosaic_slots(nullptr, 0, 0, 0, fp, ip, 5, 0, 5, 8, 3, 48, 64, &sf, ip, ip, nullptr), "slots: max_det = 0");

  // finish
  auto finish = [&](unsigned char* a, unsigned char* b, long sa, long sb, int bs, int ns, int h, int w, const unsigned char* codes, const int* len,
                    const unsigned char* atlas, int gh, int gw) { return cft_mosaic_finish(a, b, sa, sb, bs, ns, h, w, codes, len, atlas, gh, gw, nullptr); };
  EXPECT_EINVAL(finish(nullptr, nullptr, 576, 0, 5, 3, 48, 64, u, ip, u, 7, 5), "finish: null mosaic");
  EXPECT_EINVAL(finish(u, nullptr, 575, 0, 5, 3, 48, 64, u, ip, u, 7, 5), "finish: short stride");
  EXPECT_EINVAL(finish(u, u, 576, 10, 5, 3, 48, 64, u, ip, u, 7, 5), "finish: short second stride");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 5, 2, 48, 64, u, ip, u, 7, 5), "finish: ns too small");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 0, 1, 48, 64, u, ip, u, 7, 5), "finish: bs = 0");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 5, 3, 0, 64, u, ip, u, 7, 5), "finish: h = 0");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 5, 3, 48, 64, u, nullptr, u, 7, 5), "finish: names without lengths");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 5, 3, 48, 64, u, ip, nullptr, 7, 5), "finish: names without atlas");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 5, 3, 48, 64, u, ip, u, 0, 5), "finish: glyph height 0");
  EXPECT_EINVAL(finish(u, nullptr, 576, 0, 5, 3, 48, 64, u, ip, u, 7, 65), "finish: glyph width 65");

  // area
  unsigned char* dst = fake + 4096 * 32;
  EXPECT_EINVAL(cft_mosaic_area(nullptr, 192, 48, 64, dst, 96, 24, 32, nullptr), "area: null source");
  EXPECT_EINVAL(cft_mosaic_area(u, 123, 41, 41, dst, 30, 10, 10, nullptr), "area: 41 -> 10");
  EXPECT_EINVAL(cft_mosaic_area(u, 192, 48, 64, dst, 300, 49, 64, nullptr), "area: enlarges");
  EXPECT_EINVAL(cft_mosaic_area(u, 191, 48, 64, dst, 96, 24, 32, nullptr), "area: short source stride");
  EXPECT_EINVAL(cft_mosaic_area(u, 192, 48, 64, dst, 95, 24, 32, nullptr), "area: short destination stride");
  EXPECT_EINVAL(cft_mosaic_area(u, 192, 48, 64, dst, 96, 0, 32, nullptr), "area: zero height");
  EXPECT_EINVAL(cft_mosaic_area(u, 192, 48, 64, u + 192, 96, 24, 32, nullptr), "area: overlap");

  // the two new render flags
  cft_render_desc_t d;
  std::memset(&d, 0, sizeof(d));
  d.img_rgb = fake; d.h0 = 5; d.w0 = 7; d.stride_rgb = 21;
  auto render = [&](int flags) {
    return cft_detect_render(fake, &d, 1, (const int*)fake, 8, fake, 3, 0, 3, flags, fake, (const int*)fake, 8, fake, 7, 5, nullptr);
  };
  EXPECT_EINVAL(render(CFT_RENDER_CONF1), "render: tenths alone");
  EXPECT_EINVAL(render(CFT_RENDER_LABELS | CFT_RENDER_CONF1), "render: tenths without conf");
  EXPECT_EINVAL(render(CFT_RENDER_CONF | CFT_RENDER_CONF1 | CFT_RENDER_SIGNED), "render: conf without labels");
  EXPECT_EINVAL(render(16), "render: unknown flag");
  std::printf(failures ? "%d FAILED\n" : "all guards hold (%d failures)\n", failures);
  return failures != 0;
}
