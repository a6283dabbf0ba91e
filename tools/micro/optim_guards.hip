// Host-side guards and table arithmetic of cft_sgd_step / cft_ema_update under a host sanitizer, no GPU needed: every call below
// stops in the checks in front of the launch (nothing is launched, no HIP call is made) - CFT_EINVAL for a bad table, CFT_OK for a
// table without work.  The tables hold many segments of awkward sizes so that the walk over the work rows (the canonical cut) reads
// every row of a heap buffer sized exactly: an off-by-one there is what the address sanitizer is for.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/optim_guards.hip multispectral-object-detection_amd/csrc/optim.hip multispectral-object-detection_amd/csrc/runtime.hip \
//         -o tools/micro/optim_guards && tools/micro/optim_guards
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "cft_hip.h"

static int failures = 0;
#define EXPECT(call, want, what)                                                                              \
  do {                                                                                                        \
    const int st = (call);                                                                                    \
    if (st != (want)) { std::printf("FAIL %s: status %d, expected %d\n", what, st, (int)(want)); ++failures; } \
    else std::printf("ok   %-34s %s\n", what, st == CFT_OK ? "" : cft_last_error());                          \
  } while (0)

// segment rows followed by the canonical work rows, in one exactly-sized heap buffer of 8-byte words
template <typename Seg>
static std::vector<long> make_table(const std::vector<Seg>& segs, int chunk, long* nwork) {
  std::vector<cft_optim_work_t> work;
  for (size_t i = 0; i < segs.size(); ++i)
    for (long start = 0; start < segs[i].n; start += chunk) work.push_back(cft_optim_work_t{(int)i, 0, start});
  *nwork = (long)work.size();
  std::vector<long> t((segs.size() * sizeof(Seg) + work.size() * sizeof(cft_optim_work_t)) / sizeof(long));
  if (!segs.empty()) std::memcpy(t.data(), segs.data(), segs.size() * sizeof(Seg));
  if (!work.empty()) std::memcpy((char*)t.data() + segs.size() * sizeof(Seg), work.data(), work.size() * sizeof(cft_optim_work_t));
  return t;
}

template <typename Seg>
static cft_optim_work_t* work_rows(std::vector<long>& t, size_t nseg) { return (cft_optim_work_t*)((char*)t.data() + nseg * sizeof(Seg)); }

int main() {
  const int chunk = CFT_OPTIM_CHUNK;
  alignas(16) static float fake[64];          // never dereferenced: every call ends before the launch
  void* dev = fake;
  const long sizes[] = {1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2L * chunk + 3, 0, 7L * chunk};
  std::vector<cft_sgd_seg_t> sgd;
  std::vector<cft_ema_seg_t> ema;
  for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
    sgd.push_back(cft_sgd_seg_t{fake, fake + 4, fake + 8, sizes[i], (long)(i % 3)});
    ema.push_back(cft_ema_seg_t{fake, fake + 4, sizes[i]});
  }
  const int ns = (int)sgd.size();
  const float hyper[3 * 4] = {0.01f, 0.937f, 0.f, 1.f, 0.01f, 0.937f, 5e-4f, 1.f, 0.02f, 0.f, 0.f, 0.f};
  long nw = 0;
  std::vector<long> good = make_table(sgd, chunk, &nw);
  auto step = [&](const std::vector<long>& t, int nseg, long nwork, int ch, int blocks, const float* hy, int ng) {
    return cft_sgd_step(dev, t.data(), nseg, nwork, ch, blocks, hy, ng, nullptr, nullptr, nullptr);
  };
  // every guard in turn; the good table itself would launch, so it is only ever passed with something else wrong
  EXPECT(cft_sgd_step(nullptr, good.data(), ns, nw, chunk, 0, hyper, 3, nullptr, nullptr, nullptr), CFT_EINVAL, "sgd: null device table");
  EXPECT(cft_sgd_step(dev, nullptr, ns, nw, chunk, 0, hyper, 3, nullptr, nullptr, nullptr), CFT_EINVAL, "sgd: null host table");
  EXPECT(step(good, -1, nw, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: negative segment count");
  EXPECT(step(good, ns, -1, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: negative work count");
  EXPECT(step(good, ns, nw, chunk, 0, hyper, 9), CFT_EINVAL, "sgd: nine groups");
  EXPECT(step(good, ns, nw, chunk, 0, hyper, 0), CFT_EINVAL, "sgd: no group");
  EXPECT(step(good, ns, nw, chunk, 0, hyper, 2), CFT_EINVAL, "sgd: group index out of range");
  EXPECT(step(good, ns, nw, chunk, 0, nullptr, 3), CFT_EINVAL, "sgd: null hyper-parameters");
  EXPECT(step(good, ns, nw, 1000, 0, hyper, 3), CFT_EINVAL, "sgd: chunk not a multiple of 1024");
  EXPECT(step(good, ns, nw, 2 * chunk, 0, hyper, 3), CFT_EINVAL, "sgd: table cut for another chunk");
  EXPECT(step(good, ns, nw, chunk, -1, hyper, 3), CFT_EINVAL, "sgd: negative block cap");
  EXPECT(step(good, ns, nw - 1, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: one work row short");
  EXPECT(step(good, ns - 1, nw, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: one segment short");
  EXPECT(cft_sgd_step(dev, good.data(), ns, nw, chunk, 0, hyper, 3, fake + 1, (const float*)((char*)fake + 2), nullptr), CFT_EINVAL, "sgd: misaligned found_inf");
  { float h[12]; std::memcpy(h, hyper, sizeof(h)); h[11] = 1.f; EXPECT(step(good, ns, nw, chunk, 0, h, 3), CFT_EINVAL, "sgd: nesterov without momentum"); }
  { float h[12]; std::memcpy(h, hyper, sizeof(h)); h[3] = 0.5f; EXPECT(step(good, ns, nw, chunk, 0, h, 3), CFT_EINVAL, "sgd: nesterov flag 0.5"); }
  { float h[12]; std::memcpy(h, hyper, sizeof(h)); h[4] = 0.f / 0.f; EXPECT(step(good, ns, nw, chunk, 0, h, 3), CFT_EINVAL, "sgd: NaN lr"); }
  { auto s = sgd; s[4].n = -5; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: negative element count"); }
  { auto s = sgd; s[5].group = -1; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: negative group"); }
  { auto s = sgd; s[2].g = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: null gradient"); }
  { auto s = sgd; s[0].buf = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: no buffer, momentum"); }
  { auto s = sgd; s[3].p = (float*)((char*)fake + 2); long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: misaligned parameter"); }
  { auto t = good; work_rows<cft_sgd_seg_t>(t, ns)[nw - 1].start += 1; EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: last work row shifted"); }
  { auto t = good; work_rows<cft_sgd_seg_t>(t, ns)[7].seg = ns; EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: work row of segment nseg"); }
  { auto t = good; work_rows<cft_sgd_seg_t>(t, ns)[0].pad = 1; EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: padding word"); }
  { auto t = good; auto* w = work_rows<cft_sgd_seg_t>(t, ns); std::swap(w[nw - 1], w[nw - 2]); EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "sgd: work rows out of order"); }
  // tables without work are legal and launch nothing
  { std::vector<cft_sgd_seg_t> s(5, cft_sgd_seg_t{fake, fake, nullptr, 0, 2}); long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, 5, n2, chunk, 0, hyper, 3), CFT_OK, "sgd: five empty segments"); }
  { std::vector<long> t(1, 0); EXPECT(step(t, 0, 0, chunk, 0, hyper, 3), CFT_OK, "sgd: no segment"); }

  std::vector<long> egood = make_table(ema, chunk, &nw);
  auto upd = [&](const std::vector<long>& t, int nseg, long nwork, int ch, float d, float omd) {
    return cft_ema_update(dev, t.data(), nseg, nwork, ch, 0, d, omd, nullptr);
  };
  EXPECT(cft_ema_update(nullptr, egood.data(), ns, nw, chunk, 0, 0.5f, 0.5f, nullptr), CFT_EINVAL, "ema: null device table");
  EXPECT(cft_ema_update(dev, nullptr, ns, nw, chunk, 0, 0.5f, 0.5f, nullptr), CFT_EINVAL, "ema: null host table");
  EXPECT(upd(egood, -3, nw, chunk, 0.5f, 0.5f), CFT_EINVAL, "ema: negative segment count");
  EXPECT(upd(egood, ns, nw + 1 - 2, chunk, 0.5f, 0.5f), CFT_EINVAL, "ema: one work row short");
  EXPECT(upd(egood, ns, nw, 512, 0.5f, 0.5f), CFT_EINVAL, "ema: chunk 512");
  EXPECT(upd(egood, ns, nw, chunk, 0.f / 0.f, 0.5f), CFT_EINVAL, "ema: NaN decay");
  { auto s = ema; s[6].n = -1; long n2; auto t = make_table(s, chunk, &n2); EXPECT(upd(t, ns, n2, chunk, 0.5f, 0.5f), CFT_EINVAL, "ema: negative element count"); }
  { auto s = ema; s[1].m = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(upd(t, ns, n2, chunk, 0.5f, 0.5f), CFT_EINVAL, "ema: null model tensor"); }
  { auto s = ema; s[1].e = (float*)((char*)fake + 1); long n2; auto t = make_table(s, chunk, &n2); EXPECT(upd(t, ns, n2, chunk, 0.5f, 0.5f), CFT_EINVAL, "ema: misaligned tensor"); }
  { auto t = egood; work_rows<cft_ema_seg_t>(t, ns)[nw - 1].seg -= 1; EXPECT(upd(t, ns, nw, chunk, 0.5f, 0.5f), CFT_EINVAL, "ema: last work row, wrong segment"); }
  { std::vector<cft_ema_seg_t> s(3, cft_ema_seg_t{fake, fake, 0}); long n2; auto t = make_table(s, chunk, &n2); EXPECT(upd(t, 3, n2, chunk, 0.5f, 0.5f), CFT_OK, "ema: three empty segments"); }
  std::printf(failures ? "%d FAILED\n" : "all guards hold (%d failures)\n", failures);
  return failures != 0;
}
