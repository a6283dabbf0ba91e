// Host-side guards and table arithmetic of cft_adam_step under a host sanitizer, no GPU needed: every call below stops in the checks
// in front of the two launches (nothing is launched, no HIP call is made) - CFT_EINVAL for a bad argument, hyper-parameter or table,
// CFT_OK for a table without work.  The tables hold many segments of awkward sizes in heap buffers sized exactly, so that a walk past
// the last 56-byte segment row or the last work row is what the address sanitizer reports.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/adam_guards.hip multispectral-object-detection_amd/csrc/optim.hip multispectral-object-detection_amd/csrc/runtime.hip \
//         -o tools/micro/adam_guards && tools/micro/adam_guards
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
    else std::printf("ok   %-36s %s\n", what, st == CFT_OK ? "" : cft_last_error());                          \
  } while (0)

typedef cft_adam_seg_t Seg;

// segment rows followed by the canonical work rows, in one exactly-sized heap buffer of 8-byte words
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

static cft_optim_work_t* work_rows(std::vector<long>& t, size_t nseg) { return (cft_optim_work_t*)((char*)t.data() + nseg * sizeof(Seg)); }

int main() {
  static_assert(sizeof(Seg) == CFT_ADAM_SEG_BYTES, "row size");
  const int chunk = CFT_OPTIM_CHUNK;
  alignas(16) static float fake[64];          // never dereferenced: every call ends before the launch
  void* dev = fake;
  float* coef = fake + 32;
  const long sizes[] = {1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2L * chunk + 3, 0, 7L * chunk};
  std::vector<Seg> segs;
  for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i)
    segs.push_back(Seg{fake, fake + 4, fake + 8, fake + 12, fake + 16 + i, sizes[i], (long)(i % 3)});
  const int ns = (int)segs.size();
  // lr, beta1, beta2, eps, weight_decay, decoupled
  const double hyper[3 * 6] = {0.01, 0.937, 0.999, 1e-8, 0., 0., 0.01, 0.937, 0.999, 1e-8, 5e-4, 0., 0.02, 0., 0.99, 1e-3, 1e-2, 1.};
  long nw = 0;
  std::vector<long> good = make_table(segs, chunk, &nw);
  auto step = [&](const std::vector<long>& t, int nseg, long nwork, int ch, int blocks, const double* hy, int ng) {
    return cft_adam_step(dev, t.data(), nseg, nwork, ch, blocks, hy, ng, coef, nullptr, nullptr, nullptr);
  };
  auto with = [&](int at, double value, const char* what) {
    double h[18];
    std::memcpy(h, hyper, sizeof(h));
    h[at] = value;
    EXPECT(step(good, ns, nw, chunk, 0, h, 3), CFT_EINVAL, what);
  };
  // every guard in turn; the good table itself would launch, so it is only ever passed with something else wrong
  EXPECT(cft_adam_step(nullptr, good.data(), ns, nw, chunk, 0, hyper, 3, coef, nullptr, nullptr, nullptr), CFT_EINVAL, "null device table");
  EXPECT(cft_adam_step(dev, nullptr, ns, nw, chunk, 0, hyper, 3, coef, nullptr, nullptr, nullptr), CFT_EINVAL, "null host table");
  EXPECT(cft_adam_step(dev, (const char*)good.data() + 4, ns, nw, chunk, 0, hyper, 3, coef, nullptr, nullptr, nullptr), CFT_EINVAL, "host table at 4 modulo 8");
  EXPECT(step(good, -1, nw, chunk, 0, hyper, 3), CFT_EINVAL, "negative segment count");
  EXPECT(step(good, ns, -1, chunk, 0, hyper, 3), CFT_EINVAL, "negative work count");
  EXPECT(step(good, ns, nw, chunk, 0, hyper, 9), CFT_EINVAL, "nine groups");
  EXPECT(step(good, ns, nw, chunk, 0, hyper, 0), CFT_EINVAL, "no group");
  EXPECT(step(good, ns, nw, chunk, 0, hyper, 2), CFT_EINVAL, "group index out of range");
  EXPECT(step(good, ns, nw, chunk, 0, nullptr, 3), CFT_EINVAL, "null hyper-parameters");
  EXPECT(step(good, ns, nw, 1000, 0, hyper, 3), CFT_EINVAL, "chunk not a multiple of 1024");
  EXPECT(step(good, ns, nw, 2 * chunk, 0, hyper, 3), CFT_EINVAL, "table cut for another chunk");
  EXPECT(step(good, ns, nw, chunk, -1, hyper, 3), CFT_EINVAL, "negative block cap");
  EXPECT(step(good, ns, nw, chunk, 65537, hyper, 3), CFT_EINVAL, "block cap 65537");
  EXPECT(step(good, ns, nw - 1, chunk, 0, hyper, 3), CFT_EINVAL, "one work row short");
  EXPECT(step(good, ns - 1, nw, chunk, 0, hyper, 3), CFT_EINVAL, "one segment short");
  EXPECT(cft_adam_step(dev, good.data(), ns, nw, chunk, 0, hyper, 3, nullptr, nullptr, nullptr, nullptr), CFT_EINVAL, "null coef");
  EXPECT(cft_adam_step(dev, good.data(), ns, nw, chunk, 0, hyper, 3, fake + 1, nullptr, nullptr, nullptr), CFT_EINVAL, "coef at 4 modulo 8");
  EXPECT(cft_adam_step(dev, good.data(), ns, nw, chunk, 0, hyper, 3, coef, (const float*)((char*)fake + 2), nullptr, nullptr), CFT_EINVAL, "misaligned grad_scale");
  EXPECT(cft_adam_step(dev, good.data(), ns, nw, chunk, 0, hyper, 3, coef, fake + 1, (const float*)((char*)fake + 2), nullptr), CFT_EINVAL, "misaligned found_inf");
  with(6, 0. / 0., "NaN lr");
  with(2, 0. / 0., "NaN beta2");
  with(17, 0. / 0., "NaN decoupled flag");
  with(0, -1e-3, "negative lr");
  with(9, -1e-8, "negative eps");
  with(10, -5e-4, "negative weight_decay");
  with(1, 1.0, "beta1 = 1");
  with(7, -0.1, "negative beta1");
  with(14, 1.5, "beta2 = 1.5");
  with(8, -1e-9, "negative beta2");
  with(5, 0.5, "decoupled flag 0.5");
  with(11, 2.0, "decoupled flag 2");
  { auto s = segs; s[4].n = -5; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "negative element count"); }
  { auto s = segs; s[5].group = -1; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "negative group"); }
  { auto s = segs; s[ns - 1].group = 3; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "last segment in group 3 of 3"); }
  { auto s = segs; s[1].p = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "null parameter"); }
  { auto s = segs; s[2].g = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "null gradient"); }
  { auto s = segs; s[0].m = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "null exp_avg"); }
  { auto s = segs; s[11].v = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "null exp_avg_sq, empty segment"); }
  { auto s = segs; s[ns - 1].step = nullptr; long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "null step counter"); }
  { auto s = segs; s[3].p = (float*)((char*)fake + 2); long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "misaligned parameter"); }
  { auto s = segs; s[6].v = (float*)((char*)fake + 1); long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "misaligned exp_avg_sq"); }
  { auto s = segs; s[7].step = (float*)((char*)fake + 3); long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, ns, n2, chunk, 0, hyper, 3), CFT_EINVAL, "misaligned step counter"); }
  { auto t = good; work_rows(t, ns)[nw - 1].start += 1; EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "last work row shifted"); }
  { auto t = good; work_rows(t, ns)[7].seg = ns; EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "work row of segment nseg"); }
  { auto t = good; work_rows(t, ns)[0].pad = 1; EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "padding word"); }
  { auto t = good; auto* w = work_rows(t, ns); std::swap(w[nw - 1], w[nw - 2]); EXPECT(step(t, ns, nw, chunk, 0, hyper, 3), CFT_EINVAL, "work rows out of order"); }
  // tables without work are legal and launch nothing
  { std::vector<Seg> s(5, Seg{fake, fake, fake, fake, fake, 0, 2}); long n2; auto t = make_table(s, chunk, &n2); EXPECT(step(t, 5, n2, chunk, 0, hyper, 3), CFT_OK, "five empty segments"); }
  { std::vector<long> t(1, 0); EXPECT(step(t, 0, 0, chunk, 0, hyper, 3), CFT_OK, "no segment"); }
  std::printf(failures ? "%d FAILED\n" : "all guards hold (%d failures)\n", failures);
  return failures != 0;
}
