// Host-side guards of cft_detect_render / cft_detect_boxes under a host sanitizer, no GPU needed: every call below must return
// CFT_EINVAL from the checks in front of the launch (nothing is launched, no HIP call is made).  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/detect_guards.hip multispectral-object-detection_amd/csrc/detect.hip multispectral-object-detection_amd/csrc/runtime.hip \
//         -o tools/micro/detect_guards && tools/micro/detect_guards
#include <cstdio>
#include <cstring>
#include <vector>
#include "cft_hip.h"

static int failures = 0;
#define EXPECT_EINVAL(call, what)                                                           \
  do {                                                                                      \
    const int st = (call);                                                                  \
    if (st != CFT_EINVAL) { std::printf("FAIL %s: status %d\n", what, st); ++failures; }    \
    else std::printf("ok   %-28s %s\n", what, cft_last_error());                            \
  } while (0)

int main() {
  const int B = 3, max_det = 8, nc = 3;
  // never dereferenced: the guards read the host table only, and every call fails before the launch
  alignas(16) static unsigned char fake[64];
  void* dev = fake;
  std::vector<cft_render_desc_t> good(B);
  for (int b = 0; b < B; ++b) {
    std::memset(&good[b], 0, sizeof(good[b]));
    good[b].img_rgb = fake; good[b].img_ir = fake;
    good[b].h0 = 5 + b; good[b].w0 = 7 + b;
    good[b].stride_rgb = good[b].stride_ir = 3L * good[b].w0;
  }
  auto render = [&](const std::vector<cft_render_desc_t>& t, int nb, int md, int n, int color, int thick, int flags, int ld, int gh, int gw) {
    return cft_detect_render(dev, t.data(), nb, (const int*)dev, md, fake, n, color, thick, flags, fake, (const int*)dev, ld, fake, gh, gw, nullptr);
  };
  const int LC = CFT_RENDER_LABELS | CFT_RENDER_CONF;
  { auto t = good; t[2].img_rgb = nullptr; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "null image"); }
  { auto t = good; t[1].stride_rgb = 3L * t[1].w0 - 1; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "short rgb stride"); }
  { auto t = good; t[1].stride_ir = 0; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "short ir stride"); }
  { auto t = good; t[0].h0 = 0; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "zero height"); }
  { auto t = good; t[0].w0 = (1 << 24) + 1; t[0].stride_rgb = t[0].stride_ir = 1L << 30; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "width too large"); }
  { auto t = good; t[2].pad1 = 7; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "padding word"); }
  { auto t = good; t[2].stride_rgb = 1L << 41; EXPECT_EINVAL(render(t, B, max_det, nc, 0, 2, LC, 8, 7, 5), "huge stride"); }
  EXPECT_EINVAL(render(good, 0, max_det, nc, 0, 2, LC, 8, 7, 5), "B = 0");
  EXPECT_EINVAL(render(good, B, 0, nc, 0, 2, LC, 8, 7, 5), "max_det = 0");
  EXPECT_EINVAL(render(good, B, max_det, 0, 0, 2, LC, 8, 7, 5), "nc = 0");
  EXPECT_EINVAL(render(good, B, max_det, nc, 1 << 24, 2, LC, 8, 7, 5), "text colour");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 0, LC, 8, 7, 5), "thickness 0");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 65, LC, 8, 7, 5), "thickness 65");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 2, 4, 8, 7, 5), "unknown flag");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 2, CFT_RENDER_CONF, 8, 7, 5), "conf without labels");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 2, LC, 33, 7, 5), "name_ld 33");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 2, LC, 8, 0, 5), "glyph height 0");
  EXPECT_EINVAL(render(good, B, max_det, nc, 0, 2, LC, 8, 7, 65), "glyph width 65");
  EXPECT_EINVAL(cft_detect_render(dev, nullptr, B, (const int*)dev, max_det, fake, nc, 0, 2, 0, nullptr, nullptr, 0, nullptr, 0, 0, nullptr), "null host table");
  EXPECT_EINVAL(cft_detect_render(dev, good.data(), B, (const int*)(fake + 4), max_det, fake, nc, 0, 2, 0, nullptr, nullptr, 0, nullptr, 0, 0, nullptr), "misaligned boxes");
  EXPECT_EINVAL(cft_detect_render(dev, good.data(), B, (const int*)dev, max_det, fake, nc, 0, 2, CFT_RENDER_LABELS, nullptr, (const int*)dev, 8, fake, 7, 5, nullptr), "labels without names");
  const float* f = (const float*)dev;
  int* i = (int*)dev;
  EXPECT_EINVAL(cft_detect_boxes(nullptr, i, B, max_det, f, nc, 1.02f, 10.f, 0, i, i, i, nullptr), "boxes: null dets");
  EXPECT_EINVAL(cft_detect_boxes(f, i, B, max_det, f, 0, 1.02f, 10.f, 0, i, i, i, nullptr), "boxes: nc = 0");
  EXPECT_EINVAL(cft_detect_boxes(f, i, B, 1 << 30, f, nc, 1.02f, 10.f, 0, i, i, i, nullptr), "boxes: too many slots");
  EXPECT_EINVAL(cft_detect_boxes(f, i, B, max_det, f, nc, 1.02f, 10.f, 0, (int*)(fake + 8), i, i, nullptr), "boxes: misaligned out");
  EXPECT_EINVAL(cft_detect_boxes(f, i, B, max_det, f, nc, 0.f / 0.f, 10.f, 0, i, i, i, nullptr), "boxes: NaN gain");
  std::printf(failures ? "%d FAILED\n" : "all guards hold (%d failures)\n", failures);
  return failures != 0;
}
