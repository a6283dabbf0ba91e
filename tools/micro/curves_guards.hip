// Host-side guards of cft_eval_curves and cft_eval_curves_workspace_bytes under a host sanitizer, no GPU needed: every call below must
// return CFT_EINVAL from the checks in front of the first launch (nothing is launched, no HIP call is made); the grid checks read the
// caller's host copy of the FPPI grid, which is why that copy is real memory here.  Build and run on the CPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/micro/curves_guards.hip multispectral-object-detection_amd/csrc/curves.hip multispectral-object-detection_amd/csrc/metrics.hip \
//         multispectral-object-detection_amd/csrc/runtime.hip -o tools/micro/curves_guards && tools/micro/curves_guards
#include <cmath>
#include <cstdio>
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
  // device pointers are never dereferenced: every call fails before the launch
  alignas(256) static unsigned char fake[4096];
  const unsigned short* tp = (const unsigned short*)fake;
  const float* conf = (const float*)fake;
  const int* ip = (const int*)fake;
  double* dp = (double*)fake;
  int* best = (int*)fake;
  std::vector<double> grid(4096);
  for (int g = 0; g < 4096; ++g) grid[g] = 0.001 * g;
  std::vector<double> down(grid.rbegin(), grid.rend()), with_nan(grid), with_inf(grid), one_dip(grid);
  with_nan[4095] = std::nan("");
  with_inf[0] = -INFINITY;
  one_dip[4095] = one_dip[4094] - 1e-9;

  long bytes = 0;
  EXPECT_EINVAL(cft_eval_curves_workspace_bytes(100, 3, nullptr), "workspace: null result");
  EXPECT_EINVAL(cft_eval_curves_workspace_bytes(-1, 3, &bytes), "workspace: negative n");
  EXPECT_EINVAL(cft_eval_curves_workspace_bytes(1L << 30, 3, &bytes), "workspace: n = 2^30");
  EXPECT_EINVAL(cft_eval_curves_workspace_bytes(100, 0, &bytes), "workspace: nc = 0");
  EXPECT_EINVAL(cft_eval_curves_workspace_bytes(100, 65536, &bytes), "workspace: nc = 65536");
  if (cft_eval_curves_workspace_bytes(100, 3, &bytes) != CFT_OK || bytes <= 0 || (bytes & 255)) { std::printf("FAIL workspace size %ld\n", bytes); ++failures; }
  const long need = bytes;

  struct Args {
    const unsigned short* tp; const float* conf; const int* pcls; long n; const int* hist; int nc, n_images; const double* px; const double* grid;
    const double* grid_host; int ng; void* ws; long ws_bytes; double *p, *r, *f1, *py, *mr; int* best;
  };
  const Args good{tp, conf, ip, 100, ip, 3, 8, dp, dp, grid.data(), 9, fake, need, dp, dp, dp, dp, dp, best};
  auto run = [](const Args& a) {
    return cft_eval_curves(a.tp, a.conf, a.pcls, a.n, a.hist, a.nc, a.n_images, a.px, a.grid, a.grid_host, a.ng, a.ws, a.ws_bytes, a.p, a.r, a.f1,
                           a.py, a.mr, a.best, nullptr);
  };
  Args a = good;
#define BAD(field, value, what) a = good; a.field = value; EXPECT_EINVAL(run(a), what)
  BAD(tp, nullptr, "curves: null tp_bits with n > 0");
  BAD(conf, nullptr, "curves: null conf with n > 0");
  BAD(pcls, nullptr, "curves: null pcls with n > 0");
  BAD(hist, nullptr, "curves: null label_hist");
  BAD(px, nullptr, "curves: null px");
  BAD(grid, nullptr, "curves: null device grid");
  BAD(grid_host, nullptr, "curves: null host grid");
  BAD(ws, nullptr, "curves: null workspace");
  BAD(p, nullptr, "curves: null pcurve");
  BAD(r, nullptr, "curves: null rcurve");
  BAD(f1, nullptr, "curves: null f1curve");
  BAD(py, nullptr, "curves: null pycurve");
  BAD(mr, nullptr, "curves: null mr");
  BAD(best, nullptr, "curves: null best");
  BAD(n, -1, "curves: negative n");
  BAD(n, 1L << 30, "curves: n = 2^30");
  BAD(nc, 0, "curves: nc = 0");
  BAD(nc, 65536, "curves: nc = 65536");
  BAD(n_images, 0, "curves: n_images = 0");
  BAD(n_images, -2, "curves: negative n_images");
  BAD(ng, 0, "curves: empty grid");
  BAD(ng, 4097, "curves: 4097 grid values");
  BAD(ng, -1, "curves: negative grid length");
  BAD(px, (const double*)(fake + 4), "curves: misaligned px");
  BAD(mr, (double*)(fake + 12), "curves: misaligned mr");
  BAD(py, (double*)(fake + 2), "curves: misaligned pycurve");
  BAD(best, (int*)(fake + 2), "curves: misaligned best");
  BAD(conf, (const float*)(fake + 2), "curves: misaligned conf");
  BAD(tp, (const unsigned short*)(fake + 1), "curves: misaligned tp_bits");
  BAD(grid_host, (const double*)((const char*)grid.data() + 4), "curves: misaligned host grid");
  BAD(ws_bytes, need - 1, "curves: short workspace");
  BAD(ws, fake + 128, "curves: misaligned workspace");
  // the host copy of the grid is read in full (ng values, here the largest grid) before anything is launched
  a = good; a.ng = 4096; a.grid_host = down.data(); EXPECT_EINVAL(run(a), "curves: decreasing grid");
  a = good; a.ng = 4096; a.grid_host = with_nan.data(); EXPECT_EINVAL(run(a), "curves: NaN as the last value");
  a = good; a.ng = 4096; a.grid_host = with_inf.data(); EXPECT_EINVAL(run(a), "curves: -inf as the first value");
  a = good; a.ng = 4096; a.grid_host = one_dip.data(); EXPECT_EINVAL(run(a), "curves: a dip at the last value");
  std::printf(failures ? "%d FAILED\n" : "all guards hold (%d failures)\n", failures);
  return failures != 0;
}
