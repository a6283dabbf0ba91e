// Host-side guards of cft_tta_view / cft_tta_merge under a host sanitizer, no GPU needed: every call below must return CFT_EINVAL
// from the checks in front of the launch (nothing is launched, no HIP call is made).  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/tta_guards.hip multispectral-object-detection_amd/csrc/tta.hip multispectral-object-detection_amd/csrc/runtime.hip \
//         -o tools/micro/tta_guards && tools/micro/tta_guards
#include <cstdio>
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
  alignas(16) static unsigned char fake[4096];
  float* fp = (float*)fake;
  const double r83 = 0.83, r67 = 0.67, zero = 0.0, above = 1.0000001, neg = -0.5, nan = 0.0 / 0.0;

  // view: a [2, 3, 96, 64] batch; 0.83 gives 79 x 53 and 0.67 gives 64 x 42, both padded to 96 x 64
  // (96 * 0.67 = 64.32 is just above two grid cells)
  auto view = [&](const void* img, int dt, int B, int H, int W, const double* ratio, int gs, int flip, float* out, int Ho, int Wo) {
    return cft_tta_view(img, dt, B, H, W, 3L * H * W, (long)H * W, W, 1, ratio, gs, flip, out, Ho, Wo, nullptr);
  };
  EXPECT_EINVAL(view(nullptr, CFT_TTA_F32, 2, 96, 64, &r83, 32, 1, fp, 96, 64), "view: null images");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &r83, 32, 1, nullptr, 96, 64), "view: null output");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, nullptr, 32, 1, fp, 96, 64), "view: null ratio");
  EXPECT_EINVAL(view(fake, 3, 2, 96, 64, &r83, 32, 1, fp, 96, 64), "view: unknown dtype");
  EXPECT_EINVAL(view(fake + 2, CFT_TTA_F32, 2, 96, 64, &r83, 32, 1, fp, 96, 64), "view: misaligned fp32 images");
  EXPECT_EINVAL(view(fake + 1, CFT_TTA_F16, 2, 96, 64, &r83, 32, 1, fp, 96, 64), "view: misaligned fp16 images");
  EXPECT_EINVAL(view(fake, CFT_TTA_U8, 2, 96, 64, &r83, 32, 1, (float*)(fake + 4), 96, 64), "view: misaligned output");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 0, 96, 64, &r83, 32, 1, fp, 96, 64), "view: B = 0");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 0, 64, &r83, 32, 1, fp, 96, 64), "view: H = 0");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 40000, &r83, 32, 1, fp, 96, 64), "view: W too large");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &zero, 32, 1, fp, 96, 64), "view: ratio 0");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &neg, 32, 1, fp, 96, 64), "view: negative ratio");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &above, 32, 1, fp, 96, 64), "view: ratio above 1");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &nan, 32, 1, fp, 96, 64), "view: ratio NaN");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &r83, 0, 1, fp, 96, 64), "view: gs = 0");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &r83, -32, 1, fp, 96, 64), "view: negative gs");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &r83, 32, 2, fp, 96, 64), "view: flip = 2");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &r67, 32, 0, fp, 128, 64), "view: output taller than the formula");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 96, 64, &r83, 32, 0, fp, 96, 32), "view: output narrower than the formula");
  EXPECT_EINVAL(view(fake, CFT_TTA_F32, 2, 1, 64, &r67, 32, 0, fp, 32, 64), "view: scaled image empty");
  EXPECT_EINVAL(cft_tta_view(fake, CFT_TTA_F32, 2, 96, 64, -1, 6144, 64, 1, &r83, 32, 1, fp, 96, 64, nullptr), "view: negative stride");
  EXPECT_EINVAL(cft_tta_view(fake, CFT_TTA_F32, 2, 96, 64, 1L << 41, 6144, 64, 1, &r83, 32, 1, fp, 96, 64, nullptr), "view: huge stride");

  // merge: [2, 252 + 252 + 168, 8]
  alignas(16) static float arena[1 << 16];        // room for every tensor, disjoint: only the addresses are looked at
  float *y0 = arena, *y1 = arena + 5000, *y2 = arena + 10000, *out = arena + 20000;
  auto merge = [&](const float* a, const float* b, const float* c, int B, int n0, int n1, int n2, int no, float s0, float s1, float s2, int mask,
                   float w, float* o, int total) { return cft_tta_merge(a, b, c, B, n0, n1, n2, no, s0, s1, s2, mask, w, o, total, nullptr); };
  EXPECT_EINVAL(merge(nullptr, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: null view 0");
  EXPECT_EINVAL(merge(y0, y1, nullptr, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: null view 2");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, nullptr, 672), "merge: null output");
  EXPECT_EINVAL(merge(y0, (const float*)((const char*)y1 + 2), y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: misaligned view 1");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, (float*)((char*)out + 1), 672), "merge: misaligned output");
  EXPECT_EINVAL(merge(y0, y1, y2, 0, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: B = 0");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 4, 1.f, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: four columns");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 0, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 420), "merge: an empty view");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 671), "merge: rows do not add up");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.f, 0.67f, 2, 64.f, out, 672), "merge: ratio 0");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 1.5f, 2, 64.f, out, 672), "merge: ratio above 1");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, (float)nan, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: ratio NaN");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 8, 64.f, out, 672), "merge: flip bit of a fourth view");
  EXPECT_EINVAL(merge(y0, y1, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 0.f, out, 672), "merge: image width 0");
  EXPECT_EINVAL(merge(y0, out + 8, y2, 2, 252, 252, 168, 8, 1.f, 0.83f, 0.67f, 2, 64.f, out, 672), "merge: a view inside the output");
  std::printf(failures ? "%d FAILED\n" : "all guards hold (%d failures)\n", failures);
  return failures != 0;
}
