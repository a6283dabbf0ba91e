/*
 * cft_hip.h - C ABI of libcft_hip.so: the MI355X (gfx950) kernels behind the two-stream
 * YOLOv5 + CFT inference forward.
 *
 * The reference (DocF/multispectral-object-detection) has no native code and no FFI: its hot
 * path is Python nn.Modules dispatching to ATen.  Each entry point below therefore replaces
 * the ATen call sequence of one reference module forward (file:line given per function,
 * relative to /root/reference).  The Python modules in multispectral-object-detection_amd/
 * models/common.py keep the reference's class names, constructor signatures and state-dict
 * keys and call these functions through ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller; nothing is allocated or freed here;
 *  - activations are NHWC ("channels-last"): element (b,y,x,c) of a tensor with `ld` channels
 *    per pixel lives at ((b*H + y)*W + x)*ld + off + c, so a tensor may be a channel slice
 *    [off, off+C) of a wider buffer (this is how Concat / C3 / SPP avoid copies);
 *  - dtype codes: CFT_BF16 (bfloat16), CFT_F16 (IEEE half - the precision the reference's GPU callers use,
 *    test.py:66-68 `model.half()`) or CFT_F32; `dtype` is the compute/activation type; all three accumulate in fp32;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default);
 *  - return value: CFT_OK (0) or a negative CFT_E* code; nothing is launched on error.
 */
#ifndef CFT_HIP_H
#define CFT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bump with every change of a prototype below (history: csrc/runtime.hip).  The Python binding reads this line, the enums and
 * every prototype from this file: it is the only description of the ABI. */
#define CFT_ABI_VERSION 19

enum { CFT_BF16 = 0, CFT_F32 = 1, CFT_F16 = 2 };
enum { CFT_ACT_NONE = 0, CFT_ACT_SILU = 1, CFT_ACT_GELU = 2 };
enum {
  CFT_OK = 0,
  CFT_EINVAL = -1,   /* bad argument (alignment, size, dtype) */
  CFT_ELAUNCH = -2,  /* HIP launch error */
  CFT_ENODEV = -3    /* no gfx950 device / wrong architecture */
};

/* Library / device probe.  cft_abi_version() never touches the GPU. */
int cft_abi_version(void);
int cft_device_check(void);               /* CFT_OK iff the current device is gfx950 */
const char* cft_last_error(void);
/* Measurement only (bench.py's sustained leg; no reference counterpart): a one-wave kernel that spins for spin_us microseconds of the
 * constant-rate wall clock and writes out[0] = shader-clock ticks (s_memtime), out[1] = wall-clock ticks (s_memrealtime),
 * out[2] = dependent v_fma_f32 executed meanwhile, out[3] = scratch; *wall_khz = rate of the wall clock.  out: 4 x uint64 in device memory. */
int cft_clock_probe(void* out4_u64, int spin_us, int* wall_khz, void* stream);

/*
 * Convolution as implicit GEMM with fused epilogue:
 *   y[m, yoff+n] = act( sum_{kh,kw,ci} x[b, ho*s+kh-p, wo*s+kw-p, xoff+ci] * w[n][kh][kw][ci] + bias[n] )
 *                  (+ res[m, roff+n] if res != NULL),   m = (b*Ho + ho)*Wo + wo,  p = k/2
 * Replaces Conv.forward / Conv.fuseforward (models/common.py:45-50: conv2d + BatchNorm(eval,
 * folded into w/bias, utils/torch_utils.py:181-201) + SiLU), the Bottleneck residual add
 * (models/common.py:108-109), the channel concat of C3/SPP (via ldy/yoff; :142-143,:163-165),
 * nn.Linear(+bias)(+GELU)(+residual) of the CFT block (models/common.py:450-453,532-546; call
 * with B=1,H=1,W=rows,k=1) and the Detect 1x1 conv (models/yolo_test.py:46).
 *   x    : dtype, NHWC, ldx channels per pixel, slice offset xoff, cin channels used
 *   w    : dtype, [n][kpad] with (kh,kw,ci) flattened, ci fastest, zero padded to kpad
 *          (kpad % 64 == 0 for bf16, % 32 == 0 for f32; cin % 8 (bf16) / % 4 (f32) == 0)
 *   bias : float[n] or NULL
 *   res  : residual, res_dtype, ldr/roff; NULL for none.  May alias y (same element).
 *   y    : out_dtype, ldy/yoff.  n % 8 == 0, ldy % 8 == 0, yoff % 8 == 0.
 */
int cft_conv2d(const void* x, const void* w, const float* bias, const void* res, void* y,
               int B, int H, int W, int cin, int ldx, int xoff,
               int n, int kpad, int ksize, int stride,
               int ldy, int yoff, int ldr, int roff,
               int act, int dtype, int out_dtype, int res_dtype, void* stream);

/*
 * Two layers in one launch: a Conv (models/common.py:45-50, SiLU) and the pointwise Conv(s) that consume its output - in the CFT
 * networks the stride-2 Conv in front of a C3 and that C3's cv1 | cv2 (models/common.py:141-143, both read the same input and are
 * packed as one [n2][n1] weight).  y = act2(conv1x1(SiLU(conv(x)))):  the first layer's output tile is rounded to dtype in LDS and
 * becomes the second GEMM's A operand, so the n1-channel tensor between the layers is never written or read.  Results are
 * bit-identical to the two cft_conv2d launches.  x / w1 / bias1 / geometry as cft_conv2d; w2: dtype [n2][n1] (k = 1), bias2
 * float[n2] or NULL; y: dtype, ldy / yoff.  Eligible pairs only (cft_conv2d_chain_ok returns 1): bf16 / fp16, n1 == 128 (192 x 128
 * tile, two workgroups per CU, second layer's weights resident in LDS) or n1 == 256 (256 x 256 tile, 160 KiB of LDS, second
 * layer's weights streamed a K step at a time), cin % 64 == 0, kpad1 == k*k*cin, n2 <= n1; anything else is CFT_EINVAL.
 */
int cft_conv2d_chain(const void* x, const void* w1, const float* bias1, const void* w2, const float* bias2, void* y,
                     int B, int H, int W, int cin, int ldx, int xoff,
                     int n1, int kpad1, int ksize, int stride, int n2,
                     int ldy, int yoff, int act2, int dtype, void* stream);
/* 1 when cft_conv2d_chain accepts the pair (it runs the launcher's own validation, incl. the 2^31-element limits on the ldx / ldy extents). */
int cft_conv2d_chain_ok(int B, int H, int W, int cin, int ldx, int n1, int kpad1, int ksize, int stride, int n2, int ldy, int dtype);

/*
 * The chained pair with a SHORTCUT on the first layer - inside a C3 with shortcuts (models/common.py:99-109, :138-142) Bottleneck j's 3x3
 * conv and Bottleneck j+1's 1x1 conv:  y1 = SiLU(conv(x) + b1) + res  (one rounding; the Bottleneck's output AND the next shortcut),
 * y2 = act2(conv1x1(y1) + b2).  The shortcut tile is DMA-ed into the LDS images, added in fp32 before the rounding, and the images are
 * stored to y1 while the second GEMM runs: y1 is never re-read from memory and the 1x1 launch disappears.  Bit-identical to
 * cft_conv2d(x, w1, res=res) followed by cft_conv2d(y1, w2).  n1 == 256 only; otherwise the eligibility of cft_conv2d_chain_ok.
 * res: dtype, ldr / roff; y1: dtype, ldy1 / yoff1 (may alias res); y2: dtype, ldy2 / yoff2.
 */
int cft_conv2d_chain_res(const void* x, const void* w1, const float* bias1, const void* res, void* y1,
                         const void* w2, const float* bias2, void* y2,
                         int B, int H, int W, int cin, int ldx, int xoff,
                         int n1, int kpad1, int ksize, int stride, int ldr, int roff, int ldy1, int yoff1,
                         int n2, int ldy2, int yoff2, int act2, int dtype, void* stream);

/*
 * split-K nn.Linear (models/common.py:511 out_proj, :532-538 the MLP's second Linear): parts[s] (float [rows][n], s < splits) =
 * x[:, s*K/splits : (s+1)*K/splits] . w[:, same]^T (+ bias in s == 0).  For GEMMs with few output tiles and a long K loop: splits x the
 * workgroups, 1 / splits of the K steps each.  The partial sums are folded into the fp32 residual stream in a FIXED order (reproducible
 * results) by cft_layernorm_reduce.  cin % K-step == 0, kpad == cin, (kpad / K-step) % splits == 0, 2 <= splits <= 8.
 */
int cft_linear_splitk(const void* x, const void* w, const float* bias, float* parts,
                      int rows, int cin, int ldx, int n, int kpad, int splits, int dtype, void* stream);

/*
 * Bottleneck as one kernel (models/common.py:99-109 with e = 1.0, the form C3 uses :138):
 *   y = (shortcut ? x : 0) + SiLU(conv3x3(SiLU(conv1x1(x) + b1)) + b2),  c -> c -> c channels, 16-bit dtype.
 * x, y: NHWC channel slices (ldx/xoff, ldy/yoff) that must not overlap (the kernel reads a halo of x);
 * w1 [c][kpad1] and w2 [c][kpad2] in the cft_conv2d layout (BN folded).  Bit-identical to two cft_conv2d calls
 * (1x1 + SiLU, then 3x3 + SiLU + residual); the hidden tensor never reaches HBM.
 * w2_stages (required for c = 128, ignored for c = 64): the same 3x3 weights as 36 stage images of 8 KiB written by
 * cft_bottleneck_pack_w2; the kernel streams them as contiguous 1-KiB requests through a 4-slot LDS ring.
 */
int cft_bottleneck(const void* x, int ldx, int xoff, const void* w1, int kpad1, const float* b1,
                   const void* w2, int kpad2, const void* w2_stages, const float* b2, void* y, int ldy, int yoff,
                   int B, int H, int W, int c, int shortcut, int dtype, void* stream);

/* w2 [128][1152] (cft_conv2d layout of a 128 -> 128 3x3 conv) -> w2_stages: 36 x 8 KiB, stage u = k 32u .. 32u+31 of
 * every row in the order the kernel keeps it in LDS (c * kpad2 * 2 bytes, the size of w2). */
int cft_bottleneck_pack_w2(const void* w2, int kpad2, int c, void* w2_stages, int dtype, void* stream);

/* Tuning knob (A/B timing, tests): force how cft_conv2d and its relatives pick a kernel.  The ids:
 *   CFT_CONV_AUTO (0)              the automatic choice, the default;
 *   CFT_CONV_REGISTER_STAGED (1)   the register-staged 128 x 128 tile (no LDS-DMA);
 *   2, 4, 6, 7, 8, 23, 27, 30, 32, 33, 51, 60, 63, 70 - 75
 *                                  one forced tile each (the CONV_TILE_VARIANTS list of csrc/conv_gemm.hip);
 *   CFT_CONV_ASM (96)              the hand-scheduled 8-wave kernel wherever a layer is eligible, in 256-row tiles;
 *   CFT_CONV_ASM_TILE + 1 ... 4    the same in 224 / 208 / 192 / 128-row tiles (only the automatic choice picks a height by tile count);
 *   CFT_CONV_ROUND5 (97)           the automatic choice without the hand-scheduled kernels (plain and chained);
 *   CFT_CONV_GENERIC_WALK (900)    the automatic tiles on the generic address path instead of the uniform K walk.
 * The setting is PER HOST THREAD (thread_local): it reaches the launches the calling thread issues and no other's.
 * Returns the previous value (>= 0).  Any other id is refused: the setting stays as it was, cft_last_error names the id and
 * the call returns -1.  Not needed for normal use. */
enum {
  CFT_CONV_AUTO = 0,
  CFT_CONV_REGISTER_STAGED = 1,
  CFT_CONV_ASM = 96,
  CFT_CONV_ASM_TILE = 960,
  CFT_CONV_ROUND5 = 97,
  CFT_CONV_GENERIC_WALK = 900
};
int cft_set_conv_variant(int variant);

/*
 * Focus space-to-depth (models/common.py:176-179, the torch.cat of four strided slices):
 *   out[b, y, x, q*3 + c] = in[b, c, 2y+dy, 2x+dx],  q = dy + 2*dx, channels 12..15 = 0
 * in : float NCHW [B,3,H,W] contiguous (the image batch, values in [0,1)); out : dtype NHWC
 * [B,H/2,W/2,16].  The 3x3 Conv of Focus then runs through cft_conv2d with cin = 16.
 */
int cft_focus_s2d(const float* in, void* out, int B, int H, int W, int dtype, void* stream);

/*
 * Same, for the uint8 images the reference's callers hold (one [B,6,H,W] uint8 tensor: RGB = channels 0-2,
 * IR = 3-5; test.py:106-113 does `.float()/255` and the split before calling the model).  `in` points at the
 * first channel of the stream, element strides in bytes for batch / channel / row (row elements contiguous);
 * out[...] = in[...] * scale (scale = 1/255).
 */
int cft_focus_s2d_u8(const unsigned char* in, long stride_b, long stride_c, long stride_h, void* out,
                     int B, int H, int W, float scale, int dtype, void* stream);

/*
 * Focus in one kernel: the space-to-depth above plus its 3x3 Conv (+ folded BN, + SiLU; models/common.py:168-179
 * with :45-50) straight from the image, 16-bit compute (dtype = CFT_BF16 or CFT_F16), no intermediate tensor.
 * `in` is the first channel of the stream: float (in_kind = 0, scale = 1), unsigned char (in_kind = 1,
 * scale = 1/255; test.py:106-113) or half (in_kind = 2, the `img.half()` of test.py:107; dtype CFT_F16 only);
 * element strides for batch / channel / row, row elements contiguous, pointer and strides multiples of 2 elements.
 * w: dtype [n][192], k = (kh*3 + kw)*16 + ci, ci < 12 real (the cft_conv2d layout for cin = 16); n in {32,48,64,80};
 * y: dtype NHWC [B,H/2,W/2] with ldy/yoff.  Bit-identical to cft_focus_s2d(_u8) followed by cft_conv2d.
 */
int cft_focus_conv(const void* in, int in_kind, long stride_b, long stride_c, long stride_h, float scale,
                   const void* w, int kpad, const float* bias, void* y, int ldy, int yoff,
                   int B, int H, int W, int n, int act, int dtype, void* stream);

/*
 * SPP max pools (models/common.py:161-165): reads channels [0,C) of the NHWC buffer `buf`
 * (ld channels/pixel) and writes max_pool2d(k, stride 1, pad k/2) for k = k1,k2,k3 to channel
 * slices [C,2C), [2C,3C), [3C,4C) of the same buffer.  k odd, <= 13, k1 <= k2 <= k3.
 */
int cft_spp_maxpool(void* buf, int B, int H, int W, int C, int ld, int k1, int k2, int k3,
                    int dtype, void* stream);

/*
 * Channel-slice copy with optional nearest-neighbour upsampling (nn.Upsample(None,2,'nearest')
 * + Concat, yaml rows 33-34 / models/common.py:217-219):
 *   out[b, y, x, ooff + c] = in[b, y >> up, x >> up, ioff + c],  c < C;  out is [B,Ho,Wo,ldo].
 */
int cft_copy_channels(const void* in, int ldi, int ioff, void* out, int ldo, int ooff,
                      int B, int Ho, int Wo, int C, int up, int dtype, void* stream);

/*
 * Layout / dtype conversion at the boundary: any strided [B,C,H,W] tensor (in_dtype, element strides) -> NHWC
 * channel slice [ooff, ooff + cpad) of `out` in `dtype`, channels [C, cpad) zero (cpad a granule multiple).  This is what lets a module of
 * models/common.py be called with an ordinary NCHW torch tensor (as the reference's modules are) without ATen.
 */
int cft_to_nhwc(const void* in, int in_dtype, long stride_b, long stride_c, long stride_h, long stride_w,
                void* out, int ldo, int ooff, int B, int C, int cpad, int H, int W, int dtype, void* stream);

/*
 * Letterbox on the device (utils/datasets.py:1698-1728 `letterbox`: cv2.resize(INTER_LINEAR) to resized_w x resized_h,
 * then cv2.copyMakeBorder with a constant colour), 8-bit 3-channel images.  src: HWC, row stride in bytes; dst element
 * (y, x, c) at dst + y*stride_y + x*stride_x + c'*stride_c with c' = flip_channels ? 2 - c : c - strides (w*3, 3, 1) give
 * cv2's HWC image, (w, 1, h*w) with flip = 1 gives the CHW RGB plane the callers build next (datasets.py:1276-1281).
 * The geometry (resized size, top/left) is computed by the caller exactly as the reference does; colour = border value.
 */
int cft_letterbox_u8(const unsigned char* src, int src_h, int src_w, long src_row_stride,
                     unsigned char* dst, int dst_h, int dst_w, long dst_stride_y, long dst_stride_x, long dst_stride_c, int flip_channels,
                     int resized_h, int resized_w, int top, int left, int color0, int color1, int color2, void* stream);

/*
 * One launch assembles the whole uint8 [B, 6, dst_h, dst_w] batch of a non-augmented RGB + IR dataloader (RGB in planes 0-2, IR in
 * planes 3-5): per pair everything between cv2.imread and torch.from_numpy(img_all) of LoadMultiModalImagesAndLabels.__getitem__
 * (utils/datasets.py:1201-1207, :1274-1279) - the load_image_rgb_ir resize (:1361-1367), the grey letterbox border (auto=False,
 * scaleup=False: no second resize, the caller checks that) and HWC -> CHW.  The table has one cft_pair_desc_t row per pair:
 *   mode CFT_PAIR_COPY   (r == 1): h == h0, w == w0;
 *        CFT_PAIR_LINEAR (r > 1) : cv2 INTER_LINEAR for 8-bit, the arithmetic of cft_letterbox_u8, bit for bit;
 *        CFT_PAIR_AREA   (r < 1) : cv2 INTER_AREA for 8-bit: output (dy, dx) = the box average of the source over
 *                                  [dx*w0/w, (dx+1)*w0/w) x [dy*h0/h, (dy+1)*h0/h), edge cells weighted by their covered fraction
 *                                  as computeResizeAreaTab does, fp32 accumulation (columns of a row, then the rows), rounded to
 *                                  nearest; when w0 % w == 0 and h0 % h == 0 the exact integer block mean, halves rounded up.
 *   flip: 0 = the source channel order is the plane order (RGB sources, e.g. PIL), 1 = reversed (BGR sources, as cv2.imread gives).
 * desc_dev is the table in device memory (what the kernel reads), desc_host the same bytes in host memory (what the guards read:
 * every row is checked before the launch - sizes, fit, strides, mode, a reduction of at most 4x per axis, what the LDS span of a tile admits - and nothing is launched
 * on CFT_EINVAL).  dst % 4 == 0 and dst_w % 4 == 0 (rows are written as dwords); color = the border value of all three channels.
 * The sources may differ in size, mode and row stride within one launch.
 */
enum { CFT_PAIR_COPY = 0, CFT_PAIR_LINEAR = 1, CFT_PAIR_AREA = 2 };
#define CFT_PAIR_DESC_BYTES 64
#define CFT_PAIR_MAX_REDUCTION 4   /* CFT_PAIR_AREA: h0 <= 4 h and w0 <= 4 w (what one tile's source span in LDS admits) */
typedef struct {
  const unsigned char* src_rgb;   /* HWC uint8, pixels contiguous */
  const unsigned char* src_ir;
  long stride_rgb, stride_ir;     /* source row strides in bytes, >= 3 * w0 */
  int h0, w0;                     /* source size */
  int h, w;                       /* resized size */
  int top, left;                  /* where the resized image sits in the dst_h x dst_w letterbox */
  int mode, flip;
} cft_pair_desc_t;
int cft_pair_batch_u8(const void* desc_dev, const void* desc_host, int B, unsigned char* dst, int dst_h, int dst_w, int color, void* stream);

/*
 * One launch writes the whole uint8 [B, 6, dst_h, dst_w] batch of the AUGMENTED RGB + IR training loader (RGB in planes 0-2, IR in
 * planes 3-5): per item everything between the decoded originals and torch.from_numpy(img_all) of the reference's __getitem__ with
 * augment=True (utils/datasets.py:1155-1281) - the load_image_rgb_ir resize (INTER_LINEAR in both directions), the 4-tile mosaic
 * canvas of load_mosaic_RGB_IR (:1464-1603) or the grey letterbox, cv2.warpAffine of random_perspective_rgb_ir (:1819-1914),
 * augment_hsv per stream (:1374-1385), the two flips and the packing.  Every output pixel is a gather: no canvas is materialised.
 * The sources are HWC uint8 in RGB order (PIL); cv2 itself is absent, so "parity with cv2 unpinned": the raster below restates
 * OpenCV's published 8-bit paths and is defined so that the numpy restatement tests/augment_ref.py gives the same bytes.
 *
 * The table has one cft_aug_desc_t row per output image; luts is uint8 [B, 2, 3, 256] (stream RGB / IR; hue, saturation, value).
 * Output pixel (y, x) of image b, both streams:
 *   1. flips: y' = flip & CFT_AUG_FLIPUD ? dst_h - 1 - y : y,  x' = flip & CFT_AUG_FLIPLR ? dst_w - 1 - x : x.
 *   2. warp == 0: the value is canvas pixel (y', x').  warp == 1 (inv = the inverse of M[:2] that the host forms in double by
 *      warpAffine's closed form: D = 1 / (m00 m11 - m01 m10), a00 = m11 D, a01 = -m01 D, a10 = -m10 D, a11 = m00 D,
 *      a02 = -a00 m02 - a01 m12, a12 = -a10 m02 - a11 m12; inv = {a00, a01, a02, a10, a11, a12}):
 *        X = (rint(a00 * x' * 1024) + rint((a01 * y' + a02) * 1024) + 16) >> 5,  Y likewise with a10, a11, a12 (doubles, one rounding
 *        per operation, no contraction; 64-bit integers); sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
 *        value = (p(sy, sx) (32-fx)(32-fy) + p(sy, sx+1) fx (32-fy) + p(sy+1, sx) (32-fx) fy + p(sy+1, sx+1) fx fy + 512) >> 10
 *      per channel, each of the four canvas pixels p looked up on its own.
 *   3. canvas pixel (cy, cx): 114 outside [0, canvas_h) x [0, canvas_w) and outside every tile; inside tile t (cy in [y1, y2), cx in
 *      [x1, x2)) pixel (cy - padh, cx - padw) of the pair resized to (h, w): cv2 INTER_LINEAR for 8-bit from the (h0, w0) original,
 *      the arithmetic of CFT_PAIR_LINEAR bit for bit; a plain read when h == h0 and w == w0.
 *   4. HSV per stream: (r, g, b) -> 8-bit HSV: v = max, diff = v - min, s = (diff * sdiv[v] + 2048) >> 12 with sdiv[i] =
 *      rint((255 << 12) / i), sdiv[0] = 0; hh = g - b if v == r, else b - r + 2 diff if v == g, else r - g + 4 diff;
 *      h = (hh * hdiv[diff] + 2048) >> 12 (arithmetic shift) with hdiv[i] = rint((180 << 12) / (6 i)), hdiv[0] = 0; h += 180 if h < 0.
 *      Then h = lut[0][h], s = lut[1][s], v = lut[2][v], and back in float32, every operation rounded once, no contraction:
 *      sf = s / 255, vf = v / 255, hf = h / 30, k = floor(hf), f = hf - k, k = k mod 6, t0 = vf, t1 = vf (1 - sf), t2 = vf (1 - sf f),
 *      t3 = vf (1 - sf (1 - f)); (b, g, r) = (t1,t3,t0) (t1,t0,t2) (t3,t0,t1) (t0,t2,t1) (t0,t1,t3) (t2,t1,t0) for k = 0..5;
 *      each output is rint(255 t) (ties to even) saturated to 0..255.  s == 0 takes the same path (f drops out: all three are v).
 *   5. planes 0-2 = r, g, b of the RGB stream, planes 3-5 of the IR stream.
 * desc_dev / luts are device memory (what the kernel reads), desc_host the same table bytes in host memory (what the guards read:
 * every row is checked before the launch and nothing is launched on CFT_EINVAL - pointers, sizes up to CFT_AUG_MAX_SIDE, strides,
 * ntiles 1 or 4, warp / flip flags, finite coefficients below 2^20 in magnitude, every tile rectangle inside the canvas, its
 * rectangle minus its pad inside [0, h) x [0, w), no two rectangles overlapping; empty rectangles are allowed).  The kernel clamps
 * every source index it forms as well.  dst % 4 == 0 and dst_w % 4 == 0 (a thread stores 4 pixels of a plane as one dword).  No
 * atomics: every output byte is written once by one thread.
 */
enum { CFT_AUG_FLIPLR = 1, CFT_AUG_FLIPUD = 2 };
#define CFT_AUG_DESC_BYTES 400
#define CFT_AUG_TILE_BYTES 80
#define CFT_AUG_MAX_SIDE 16384   /* every image, canvas and output side: coordinates in 1/1024 pixel stay far inside 64 bits and the float taps exact */
typedef struct {
  const unsigned char* src_rgb;   /* HWC uint8 in RGB order, pixels contiguous */
  const unsigned char* src_ir;
  long stride_rgb, stride_ir;     /* source row strides in bytes, >= 3 * w0 */
  int h0, w0;                     /* source size */
  int h, w;                       /* resized size */
  int x1, y1, x2, y2;             /* the tile's rectangle in the canvas, [x1, x2) x [y1, y2) */
  int padw, padh;                 /* canvas (cy, cx) is resized pixel (cy - padh, cx - padw) */
  int reserved[2];
} cft_aug_tile_t;
typedef struct {
  int ntiles;                     /* 1 (letterbox) or 4 (mosaic) */
  int warp;                       /* 0: output = canvas, 1: output = warpAffine of the canvas through inv */
  int canvas_h, canvas_w;
  int flip;                       /* CFT_AUG_FLIPLR | CFT_AUG_FLIPUD */
  int reserved[3];
  double inv[6];                  /* a00 a01 a02 a10 a11 a12 */
  cft_aug_tile_t tile[4];
} cft_aug_desc_t;
int cft_augment_batch_u8(const void* desc_dev, const void* desc_host, const unsigned char* luts, int B, unsigned char* dst, int dst_h, int dst_w, void* stream);

/*
 * Baseline JPEG decoding in two halves (no reference counterpart: the reference hands every file to cv2.imread).  The yardstick is
 * PIL's decode of the same bytes (libjpeg-turbo, JDCT_ISLOW, fancy upsampling), np.array(Image.open(f).convert('RGB')), byte for byte.
 *
 * HOST half - plain C++, no HIP call, no GPU needed, re-entrant: no shared mutable state, not even cft_last_error's text; results
 * travel in the return code and in caller memory, so many threads may call it at once.  Neither function reads past nbytes or writes
 * past the sizes cft_jpeg_info reported, whatever the bytes are.
 *   cft_jpeg_info(bytes, nbytes, info): parses the markers up to SOS and fills a cft_jpeg_info_t (host, CFT_JPEG_INFO_BYTES).
 *   cft_jpeg_entropy(bytes, nbytes, coef, qtab, info): Huffman-decodes the single interleaved scan into QUANTISED int16 coefficients:
 *     coef holds info->ncoef values, component after component (component c starts at 64 * sum_{k<c} bw[k] * bh[k]), blocks in
 *     raster order of the component's bw x bh grid, 64 values per block in natural (de-zigzagged) order; every value is written.
 *     qtab: uint16 [3][64], the quantisation table of each component in natural order (rows of absent components are zero).
 *     info: what cft_jpeg_info returned for the same bytes (checked against the file again: CFT_EINVAL when it differs).
 *   Return: CFT_OK, CFT_EINVAL (null pointer, nbytes < 1, info of another file) or CFT_JPEG_UNSUPPORTED: the file is outside the subset
 *   and the caller decodes it with PIL.  Supported: SOF0, 8-bit samples, 8-bit quantisation tables, one scan holding every component,
 *   sides 1..CFT_JPEG_MAX_SIDE; 1 component sampled 1x1, or 3 components with luma 1x1, 2x1 or 2x2 (h x v) and chroma 1x1; JFIF or no
 *   colour marker, or an Adobe marker with transform 1.  Unsupported: anything else - not a JPEG, an Adobe marker with another transform,
 *   component ids 'R' 'G' 'B' without a JFIF marker, 4 components, progressive / arithmetic / 12-bit coding, a DNL marker, no EOI after
 *   the scan, a wrong or missing restart marker, truncated or corrupt entropy data, any coefficient with |coef| * q > 32767 - and a
 *   chroma component halved horizontally whose downsampled width is <= 2, where libjpeg replicates pixels instead of filtering (kept
 *   when that width is 1 and the component is one row high or not halved vertically: both methods then give the same bytes).
 *
 * DEVICE half - cft_jpeg_decode_u8 decodes n images in one call: two launches on the stream, no atomics, every output byte written
 * once.  table_dev (device) / table_host (host, the same bytes, what the guards read) hold one cft_jpeg_desc_t row per image.  Every
 * row is checked before the launch and nothing is launched on CFT_EINVAL: null or misaligned pointers (coef 2, qtab 2, plane_off and
 * the workspace 16), sides 1..CFT_JPEG_MAX_SIDE, sampling in the subset, bw / bh equal to the padded block grid of that geometry,
 * dst_stride >= 3 * width, [plane_off, plane_off + 64 * blocks) inside workspace_bytes and at or after the end of the previous
 * row's range (the ranges ascend, so no two overlap).
 * 1 <= n <= 65535.  The kernels clamp their own indices as well.
 *   1. jpeg_idct_kernel, 8 lanes per 8x8 block: dequantise (coef * q, int32), then libjpeg's jpeg_idct_islow (CONST_BITS 13,
 *      PASS1_BITS 2; FIX constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172; the published butterfly):
 *      columns first, descaled by 11, the transpose through LDS, then rows, descaled by 18, DESCALE(x, n) = (x + (1 << (n-1))) >> n,
 *      + 128, saturated to 0..255.  A lane stores the 8 bytes of its row as one 8-byte word into the component's plane in the
 *      workspace: component c is a (8 bh[c]) x (8 bw[c]) byte plane at plane_off + 64 * sum_{k<c} bw[k] * bh[k], row stride 8 bw[c].
 *   2. jpeg_colour_kernel, one thread per 4 consecutive pixels of an output row.  Chroma is upsampled over the component's
 *      DOWNSAMPLED size cw x ch = ceil(width * h / hmax) x ceil(height * v / vmax); the padding samples of the IDCT are never read:
 *      every neighbour index is clamped into [0, cw) x [0, ch), which is what the edge rules below amount to.
 *        h2v1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, out[0] = in[0], out[2 cw - 1] = in[cw-1].
 *        h2v2: the neighbouring row is the one above for an even output row, the one below for an odd one (at the top and bottom the
 *              component's own first / last row); s[i] = 3 in_row[i] + in_neighbour[i]; out[2i] = (3 s[i] + s[i-1] + 8) >> 4,
 *              out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4; the first output is (4 s[0] + 8) >> 4, the last (4 s[cw-1] + 7) >> 4.
 *      Colour, cb and cr centred at 128, arithmetic shifts, results clamped to 0..255:
 *        R = Y + ((91881 cr + 32768) >> 16),  B = Y + ((116130 cb + 32768) >> 16),  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16).
 *      One component: R = G = B = Y (what convert('RGB') does to mode L).  dst is HWC RGB uint8, pixel (y, x) at dst + y * dst_stride + 3 x.
 */
#define CFT_JPEG_UNSUPPORTED 1
#define CFT_JPEG_MAX_SIDE 16384
#define CFT_JPEG_INFO_BYTES 128
#define CFT_JPEG_DESC_BYTES 96
#define CFT_JPEG_QTAB_BYTES 384
typedef struct {
  int width, height;
  int ncomp;                      /* 1 or 3 */
  int hmax, vmax;                 /* the luma sampling factors */
  int mcus_x, mcus_y;
  int restart_interval;           /* MCUs between restart markers, 0 = none */
  int hs[3], vs[3];               /* per component: sampling factors, */
  int bw[3], bh[3];               /*   block grid padded to whole MCUs, */
  int cw[3], ch[3];               /*   downsampled size in samples */
  int reserved[2];
  long ncoef;                     /* int16 coefficients of the file: 64 * sum bw * bh */
  long plane_bytes;               /* bytes of plane workspace: 64 * sum bw * bh */
} cft_jpeg_info_t;
typedef struct {
  const short* coef;              /* device: what cft_jpeg_entropy wrote */
  const unsigned short* qtab;     /* device: uint16 [3][64] */
  unsigned char* dst;             /* device: HWC RGB uint8 */
  long dst_stride;                /* bytes per row of dst, >= 3 * width */
  long plane_off;                 /* where this image's planes start in the workspace, a multiple of 16 */
  int width, height;
  int ncomp, hmax, vmax;
  int bw[3], bh[3];
  int reserved[3];
} cft_jpeg_desc_t;
int cft_jpeg_info(const unsigned char* bytes, long nbytes, cft_jpeg_info_t* info);
int cft_jpeg_entropy(const unsigned char* bytes, long nbytes, short* coef, unsigned short* qtab, const cft_jpeg_info_t* info);
int cft_jpeg_decode_u8(const void* table_dev, const void* table_host, int n, void* workspace, long workspace_bytes, void* stream);

/*
 * Baseline JPEG ENCODING, the decoder's two halves in the other direction (csrc/jpeg_encode.hip; no reference counterpart: the
 * reference writes its files with cv2.imwrite).  The yardstick is PIL, Image.fromarray(a).save(f, 'JPEG', quality=q, subsampling=s)
 * with optimize off (libjpeg-turbo, JDCT_ISLOW, the standard Huffman tables): the device half is checked on quantised coefficients
 * (cft_jpeg_entropy of PIL's file), the whole file on bytes.  All arithmetic is integer, every shift arithmetic.
 *   1. Colour (3 components): Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16,
 *      Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 *      One component: the grey byte is Y.
 *   2. Edges and downsampling.  A full-resolution sample outside the image is the nearest one inside: x clamped to width - 1, y to
 *      height - 1.  A component halved horizontally (h2v1) is out[i] = (in[2i] + in[2i+1] + bias) >> 1 with bias 0, 1, 0, 1 ... by
 *      output column i; halved both ways (h2v2) out[i] = (the 2 x 2 samples + bias) >> 2 with bias 1, 2, 1, 2 ...  Columns are NOT clamped
 *      to the downsampled width cw: the padded column i >= cw averages clamped full-resolution samples with its own bias.  Rows are:
 *      a row >= ch = ceil(height * v / vmax) of a component repeats its last DOWNSAMPLED row ch - 1 (for an even height that is the
 *      mean of the last two rows, not the last row).
 *   3. Forward DCT: libjpeg's jpeg_fdct_islow on samples - 128 (CONST_BITS 13, PASS1_BITS 2, the twelve FIX constants of the decoder
 *      above, the published butterfly).  Rows first: outputs 0 and 4 are (sum) << 2, the others DESCALE(x, 11); then columns: outputs
 *      0 and 4 are DESCALE(x, 2), the others DESCALE(x, 15).  DESCALE(x, n) = (x + (1 << (n-1))) >> n.  The result is 8 x the DCT.
 *   4. Quantise: d = q << 3, coef = sign(c) * ((|c| + (d >> 1)) / d), the division truncating (done as an unsigned integer division).
 *   5. Tables: scale = quality < 50 ? 5000 / quality : 200 - 2 quality, q = clamp((base * scale + 50) / 100, 1, 255) over the luminance
 *      and chrominance tables of ITU T.81 Annex K, quality 1..100.  The four Huffman tables are Annex K's.
 *   6. Dummy blocks: a block of the MCU-padded grid bw x bh outside the component's real grid ceil(cw / 8) x ceil(ch / 8) is not
 *      transformed; it is coded with all AC zero and the DC of the previous block of its component in MCU order (a DC difference of
 *      0).  Only luma has them, under subsampling.  The device writes 64 zeros there, the writer ignores what the buffer holds there.
 *   7. File: SOI, APP0 JFIF 1.01 (units 0, density 1 x 1, no thumbnail), DQT luma, DQT chroma (3 components only), SOF0 (component ids
 *      1 2 3, chroma sampled 1x1 on table 1), DHT DC0, AC0, DC1, AC1 (one component: DC0, AC0), SOS, one interleaved scan without
 *      restart markers, 0xFF bytes stuffed, the last byte padded with 1-bits, EOI.
 *
 * HOST half - plain C++, no HIP call, re-entrant as the decoder's host half is (nothing shared is written, not even cft_last_error's
 * text).  Sampling is the decoder's subset: 1 component 1x1; 3 components with luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0).
 *   cft_jpeg_layout(width, height, ncomp, hmax, vmax, info): the cft_jpeg_info_t of a file to be written (what cft_jpeg_info reports
 *     for PIL's file of that geometry; restart_interval 0).  CFT_EINVAL: null info, sides outside 1..CFT_JPEG_MAX_SIDE, other sampling.
 *   cft_jpeg_quality_tables(quality, qtab): uint16 [3][64] in natural order, row 0 luminance, rows 1 and 2 chrominance.  CFT_EINVAL:
 *     null pointer, quality outside 1..100.
 *   cft_jpeg_write_bound(info, bound): *bound receives a byte count no file of that geometry exceeds (headers + 416 bytes per block:
 *     63 AC symbols of 16 + 10 bits and a DC of 11 + 11 bits, every byte stuffed; beyond 2^31 for the largest sides, hence a long).
 *     CFT_EINVAL, with *bound = -1, for a null pointer or an info that cft_jpeg_layout would not have produced.
 *   cft_jpeg_write(coef, qtab, info, out, cap, nbytes): headers and Huffman coding of coef (the layout cft_jpeg_entropy writes and
 *     cft_jpeg_encode_coef produces) into out[0, cap); *nbytes receives the file size.  Never writes at or past out + cap.  Return:
 *     CFT_OK; CFT_EINVAL (null pointer, info that cft_jpeg_layout would not have produced, a table entry outside 1..255 or chroma rows
 *     that differ, cap < 0); CFT_JPEG_SHORT_BUFFER (cap too small: *nbytes is 0, out holds a prefix); CFT_JPEG_UNSUPPORTED (a
 *     coefficient baseline coding cannot hold: an AC value beyond 10 bits or a DC difference beyond 11).
 *
 * DEVICE half - cft_jpeg_encode_coef turns n images of mixed sizes into quantised coefficients in ONE launch, grid (blocks of the
 * largest image / 32, image): jpeg_fdct_kernel, 8 lanes per 8x8 block of the padded grids of all components; lane r gathers row r of
 * its block straight from the source (colour conversion and downsampling on the way, indices clamped as in 2.), transforms it, the
 * block is transposed through LDS (72-dword block stride), lane c transforms and quantises column c, a second LDS transpose hands
 * lane r the 8 coefficients of row r, stored as one 16-byte word.  No plane workspace, no atomics, no inline assembly; every
 * coefficient of the padded grid is written once (dummy blocks as zeros).  table_dev / table_host hold one cft_jpeg_enc_desc_t per
 * image (device copy / host copy of the same bytes).  Every row of the host copy is checked before the launch and nothing is
 * launched on CFT_EINVAL: null pointers, misaligned ones (tables 8, coef 16, qtab and qtab_host 2), 1 <= n <= 65535, sides
 * 1..CFT_JPEG_MAX_SIDE, sampling in the subset, src_stride >= ncomp * width, bw / bh equal to the padded grid, every entry of
 * qtab_host rows < ncomp in 1..255.  The kernel clamps its own indices as well and treats a zero divisor as 1.
 * src: HWC uint8, RGB or one channel, pixel (y, x) at src + y * src_stride + ncomp * x; it is only read.
 */
#define CFT_JPEG_SHORT_BUFFER 2
#define CFT_JPEG_ENC_DESC_BYTES 96
typedef struct {
  const unsigned char* src;       /* device: HWC uint8, 3 channels RGB or 1 */
  const unsigned short* qtab;     /* device: uint16 [3][64], natural order */
  const unsigned short* qtab_host;/* host: the same tables, what the guards read */
  short* coef;                    /* device: 64 * sum bw * bh int16, 16-byte aligned */
  long src_stride;                /* bytes per row of src, >= ncomp * width */
  int width, height;
  int ncomp, hmax, vmax;
  int bw[3], bh[3];
  int reserved[3];
} cft_jpeg_enc_desc_t;
int cft_jpeg_layout(int width, int height, int ncomp, int hmax, int vmax, cft_jpeg_info_t* info);
int cft_jpeg_quality_tables(int quality, unsigned short* qtab);
int cft_jpeg_write_bound(const cft_jpeg_info_t* info, long* bound);
int cft_jpeg_write(const short* coef, const unsigned short* qtab, const cft_jpeg_info_t* info, unsigned char* out, long cap, long* nbytes);
int cft_jpeg_encode_coef(const void* table_dev, const void* table_host, int n, void* stream);

/* Elementwise out = a + b over M pixels x C channels (Add / Add2, models/common.py:228-243). */
int cft_add(const void* a, int lda, int aoff, const void* b, int ldb, int boff,
            void* out, int ldo, int ooff, long M, int C, int dtype, void* stream);

/*
 * CFT tokeniser (models/common.py:608-621): AdaptiveAvgPool2d((8,8)) of both streams, flatten,
 * concat on the token axis (RGB tokens 0..63, IR tokens 64..127), + pos_emb.
 *   tokens[b, s*64 + i*8 + j, c] = mean(window(i,j) of stream s)[c] + pos_emb[s*64+i*8+j, c]
 * window rows [floor(i*H/8), ceil((i+1)*H/8)).  rgb/ir: dtype NHWC; tokens: float [B,128,C].
 */
int cft_gpt_tokenize(const void* rgb, int ld_rgb, int off_rgb, const void* ir, int ld_ir, int off_ir,
                     const float* pos_emb, float* tokens, int B, int H, int W, int C,
                     int dtype, void* stream);

/* LayerNorm over the last dim (eps 1e-5, affine; models/common.py:529-530,572):
 * x float [rows, C] -> y out_dtype [rows, C]. */
int cft_layernorm(const float* x, const float* gamma, const float* beta, void* y,
                  long rows, int C, float eps, int out_dtype, void* stream);
/* x (float [rows, C], updated in place) += parts[0] + ... + parts[nparts-1] (float [nparts][rows][C], cft_linear_splitk), then
 * y = LayerNorm(x): the residual add of models/common.py:543-544 and the LayerNorm of the next sub-block (:529-530, :572) in one pass. */
int cft_layernorm_reduce(float* x, const float* parts, int nparts, const float* gamma, const float* beta, void* y,
                         long rows, int C, float eps, int out_dtype, void* stream);

/*
 * Multi-head self-attention core (models/common.py:491-510): for each (b, head)
 *   O = softmax(Q K^T / sqrt(dk)) V  over T = 128 tokens.
 * qkv : dtype [B*128, 3*heads*dkp]: row = token, columns [which(q,k,v)][head][dkp]; dkp is the
 * head width padded with zeros to a multiple of 32 (bf16) / 16 (f32); dk the true head width.
 * out : dtype [B*128, heads*dkp].
 * attn_pdrop / seed: training-mode dropout of the attention probabilities (models/common.py:507 `attn_drop`), applied
 * inside the kernel with the counter-based mask of cft_dropout; 0 = inference.
 */
int cft_attention(const void* qkv, void* out, int B, int heads, int dk, int dkp,
                  int dtype, float attn_pdrop, unsigned long long seed, void* stream);

/*
 * CFT de-tokeniser fused with the residual add (models/common.py:626-637 + Add2 :238-243):
 *   out[b,y,x,c] = (base ? base[b,y,x,c] : 0) + bilinear_{8x8 -> HxW, align_corners=False}(tokens[b, s*64 + ., c])
 * tokens: float [B,128,C] (already through ln_f); s selects the stream (0 RGB, 1 IR).
 */
int cft_gpt_upsample_add(const float* tokens, int s, const void* base, int ldb, int boff,
                         void* out, int ldo, int ooff, int B, int H, int W, int C,
                         int dtype, void* stream);

/*
 * The same for BOTH streams of a CFT block in one launch, plus the Add that consumes the two results (models/common.py:626-637 twice,
 * Add2 :238-243 twice, Add :228-229):  out0 = base0 + up(tokens[:, :64]), out1 = base1 + up(tokens[:, 64:]),
 * sum (may be NULL) = out0 + out1 formed in fp32 before the one rounding.  out0 / out1 are bit-identical to two cft_gpt_upsample_add calls.
 */
int cft_gpt_upsample_add2(const float* tokens, const void* base0, int ldb0, int boff0, const void* base1, int ldb1, int boff1,
                          void* out0, int ldo0, int ooff0, void* out1, int ldo1, int ooff1, void* sum, int lds, int soff,
                          int B, int H, int W, int C, int dtype, void* stream);

/*
 * The CFT block on a vert_anchors x horz_anchors grid (models/common.py:549-639 with GPT(..., vert_anchors=va, horz_anchors=ha)):
 * T = 2 * va * ha tokens, RGB cells 0 .. va*ha-1 then IR, row-major within a stream.  Supported: 1 <= va, ha, va * ha <= 1024.
 * At (8, 8) each entry point below is bit-identical to its 8x8 counterpart above.
 *
 * Tokeniser (replaces the AdaptiveAvgPool2d((va, ha)) + flatten + cat + pos_emb of models/common.py:606-621):
 *   tokens[b, s*va*ha + i*ha + j, c] = mean(window(i,j) of stream s)[c] + pos_emb[s*va*ha + i*ha + j, c]
 * window rows [floor(i*H/va), ceil((i+1)*H/va)), columns [floor(j*W/ha), ceil((j+1)*W/ha)) (overlapping when H < va or W < ha).
 * rgb/ir: dtype NHWC; pos_emb float [2*va*ha, C]; tokens: float [B, 2*va*ha, C].
 */
int cft_gpt_tokenize_grid(const void* rgb, int ld_rgb, int off_rgb, const void* ir, int ld_ir, int off_ir,
                          const float* pos_emb, float* tokens, int B, int H, int W, int C, int va, int ha,
                          int dtype, void* stream);

/*
 * Multi-head self-attention core over any token count 1 <= T <= 2048 (models/common.py:491-510), flash-style (64-key tiles, online
 * softmax; numerics in csrc/attention_tokens.hip).  qkv : dtype [B*T, 3*heads*dkp], out : dtype [B*T, heads*dkp], the layout of
 * cft_attention.  Training dropout index ((b*heads + h)*T + q)*T + k (cft_attention's at T = 128).
 */
int cft_attention_tokens(const void* qkv, void* out, int B, int T, int heads, int dk, int dkp,
                         int dtype, float attn_pdrop, unsigned long long seed, void* stream);

/*
 * De-tokeniser on a va x ha grid (models/common.py:626-637 + Add2 :238-243): cft_gpt_upsample_add with
 * bilinear_{va x ha -> H x W, align_corners=False}; tokens float [B, 2*va*ha, C], contiguous, 16-byte aligned.
 */
int cft_gpt_upsample_add_grid(const float* tokens, int s, const void* base, int ldb, int boff,
                              void* out, int ldo, int ooff, int B, int H, int W, int C, int va, int ha,
                              int dtype, void* stream);

/* Both streams + Add2 twice (+ Add, models/common.py:228-229) on a va x ha grid: cft_gpt_upsample_add2 with the grid above. */
int cft_gpt_upsample_add2_grid(const float* tokens, const void* base0, int ldb0, int boff0, const void* base1, int ldb1, int boff1,
                               void* out0, int ldo0, int ooff0, void* out1, int ldo1, int ooff1, void* sum, int lds, int soff,
                               int B, int H, int W, int C, int va, int ha, int dtype, void* stream);

/*
 * Detect decode (models/yolo_test.py:47-57).  logits: float [B,ny,nx,ldl] holding na*no valid
 * channels (channel = a*no + o), the output of the 1x1 conv.  Writes
 *   raw [B,na,ny,nx,no]            = logits permuted (the reference's x[i])
 *   pred[B, row0 + (a*ny+y)*nx+x, o] with total_rows rows per image:
 *        xy = (2*sig - 0.5 + grid) * stride,  wh = (2*sig)^2 * anchor[a],  rest = sig
 * anchors: float[na*2] in pixels (anchor_grid of this level).
 */
int cft_detect_decode(const float* logits, int ldl, float* raw, float* pred, const float* anchors,
                      int B, int ny, int nx, int na, int no, float stride,
                      long row0, long total_rows, void* stream);

/*
 * Training-mode forward (forward only, no autograd).
 *
 * cft_batchnorm_train: BatchNorm2d with BATCH statistics on the fp32 conv output x [M, ldx] (channels xoff..xoff+C), as
 * `act(bn(conv(x)))` does when `bn.training` (models/common.py:45-47): biased variance for the normalisation, running
 * statistics updated in place with `momentum` and the unbiased variance (torch semantics; NULL = do not track), then
 * SiLU / none, optional residual add (Bottleneck shortcut, :108-109) and the store into an NHWC channel slice in
 * `out_dtype`.  workspace: cft_batchnorm_train_workspace(M, C) bytes of device memory.
 *
 * cft_dropout: in-place nn.Dropout(p) in training mode on a contiguous tensor of n elements (GPT.drop :611, resid_drop
 * :511, the MLP's Dropout :537): element i is kept iff hash(seed, i) >= p * 2^32 and scaled by 1/(1-p).  x is 16-byte aligned; n > 0
 * need not be a multiple of the 16-byte granule: the last n % granule elements are moved byte-exactly, nothing past element n is touched.
 */
long cft_batchnorm_train_workspace(long M, int C);
int cft_batchnorm_train(const float* x, int ldx, int xoff, long M, int C,
                        const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float momentum, float eps, const void* res, int ldr, int roff, int res_dtype,
                        void* y, int ldy, int yoff, int act, int out_dtype,
                        void* workspace, long workspace_bytes, void* stream);
int cft_dropout(void* x, long n, float p, unsigned long long seed, int dtype, void* stream);

/*
 * Batched NMS on the decoded predictions (utils/general.py:455-543 `non_max_suppression`, incl. the
 * torchvision.ops.nms call at :527): per image keep rows with obj > conf_thres, conf = obj*cls, best class
 * (multi_label = 0) or every class above conf_thres (multi_label = 1), optional class filter (class_allow:
 * device array of no-5 bytes, non-zero = class kept, :505-506; NULL = all classes), xywh -> xyxy, the max_nms
 * pre-truncation to the highest confidences (:469,:515-516; 0 = off), per-class greedy NMS (class offset
 * 4096 px unless agnostic) with IoU > iou_thres suppression, at most max_det detections.
 *   pred    : float [B, rows, no]            dets : float [B, max_det, 6] (x1,y1,x2,y2,conf,cls), first counts[b] rows valid,
 *                                                   the others zeroed
 *   scratch : >= B * round_up(rows * (multi_label ? no-5 : 1), 4) * 32 bytes of device memory, 16-byte aligned
 */
int cft_nms(const float* pred, int B, int rows, int no, float conf_thres, float iou_thres,
            int agnostic, int multi_label, const unsigned char* class_allow, int max_det, int max_nms,
            void* scratch, long scratch_bytes, float* dets, int* counts, void* stream);

/*
 * mAP statistics of test.py on the GPU.
 *
 * cft_eval_match replaces the per-image loop of test.py:132-218 (labels to pixels :125, xywh2xyxy + scale_coords of the
 * labels :201-202 and of the predictions :148-149, box_iou :207 and the greedy per-class matching :204-218).  Two launches:
 * a stable grouping of the labels by image, then one workgroup per image.
 *   dets [B, max_det, 6] / counts [B] : the cft_nms output (device; never read on the host)
 *   targets [nt, 6]                   : image index, class, x, y, w, h normalised to the img_h x img_w letterbox (device)
 *   geom [B, 5]                       : h0, w0, gain, padw, padh per image, float32 (device; scale_coords, utils/general.py:353-366)
 *   iouv_host [niou]                  : the IoU thresholds, HOST memory, copied into the launch (niou <= 16)
 * Writes, per slot (b, r) of [B, max_det]: tp_bits (bit k = correct[:, k]), conf (or NULL), pcls (int class, 0 if single_cls,
 * -1 for r >= counts[b]; or NULL) and optionally correct [B, max_det, niou] bytes.  label_hist (int [nc + 1], or NULL) is ADDED
 * to: per-class label counts, slot nc = labels whose class is not an integer in [0, nc).  tcls [nt] / nl [B] (or NULL) receive
 * the label classes grouped by image in target order and the label count of each image.
 * workspace: >= cft_eval_match_workspace_bytes(B, nt) bytes, 256-byte aligned.  No allocation, no synchronisation.
 */
long cft_eval_match_workspace_bytes(int B, int nt);
int cft_eval_match(const float* dets, const int* counts, int B, int max_det, const float* targets, int nt, int img_h, int img_w,
                   const float* geom, const float* iouv_host, int niou, int single_cls, void* workspace, long workspace_bytes,
                   unsigned char* correct, unsigned short* tp_bits, float* conf, int* pcls, int* label_hist, int nc,
                   int* tcls, int* nl, void* stream);

/*
 * cft_eval_ap replaces ap_per_class (utils/metrics.py:18-79) and compute_ap (:82-108) over n accumulated detections:
 * a stable LSD radix sort by (class, conf descending; ties in insertion order), exact integer TP / FP counts, recall and
 * precision in float64, p / r at the 1000 px points and the 101-point interpolated AP with numpy's np.interp rule, f1 and
 * the argmax of its class mean.  Classes are those with label_hist[c] > 0 (np.unique(target_cls)); detections of other
 * classes (or pcls outside [0, nc)) are dropped.
 *   tp_bits [n] (bit k = IoU column k), conf [n] float, pcls [n] int, label_hist [nc] int  (device)
 *   px [1000], x [101] : the float64 grids np.linspace(0, 1, 1000) and np.linspace(0, 1, 101) (device)
 *   out [nc * (4 + niou)] float64 (device) = p[nc] | r[nc] | f1[nc] | ntp[nc] (TPs in column 0) | ap[nc, niou];
 *   rows of classes without labels are 0.
 * workspace: >= cft_eval_ap_workspace_bytes(n, nc) bytes, 256-byte aligned.  No allocation, no synchronisation.
 */
long cft_eval_ap_workspace_bytes(long n, int nc);
int cft_eval_ap(const unsigned short* tp_bits, const float* conf, const int* pcls, long n, int niou, const int* label_hist, int nc,
                const double* px, const double* x, void* workspace, long workspace_bytes, double* out, void* stream);

/*
 * cft_eval_curves: the curves of a validation run over the same n accumulated detections, sorted as cft_eval_ap sorts them (the
 * call sorts by itself: it needs no preceding cft_eval_ap and leaves that call's results alone).  All at IoU column 0 (bit 0 of
 * tp_bits), float64, one row per class c in [0, nc); rows of classes with label_hist[c] <= 0 are zero.
 *   pcurve, rcurve, f1curve [nc, 1000] : precision, recall and f1 = 2 p r / (p + r + 1e-16) at the px points, np.interp(-px, -conf, .)
 *       with left = 1 / 0 (utils/metrics.py:57, :61, :70): what plot=True draws as P_curve, R_curve and F1_curve.
 *   pycurve [nc, 1000] : np.interp(px, mrec, mpre) with compute_ap's arrays (:67, :93-97; sentinels 0 and recall[-1] + 0.01, 1 and
 *       0, reverse running maximum): PR_curve.  A class with labels and no predictions has a row of zeros (the reference appends
 *       no row for it).
 *   best [1] int : the index of f1.mean(0).argmax() over the classes with labels (:77), first index on ties, a NaN wins; the index
 *       at which cft_eval_ap reads its p, r and f1.
 *   mr [nc, ng] : the miss rate at each value of fppi_grid.  With n_l = label_hist[c] and the class's predictions by descending
 *       conf (ties in insertion order): tpc[k] = TPs among the first k + 1, fpc[k] = k + 1 - tpc[k], fppi[k] = fpc[k] / n_images,
 *       miss[k] = 1 - tpc[k] / (n_l + 1e-16), preceded by the sentinel fppi = -1, miss = 1; mr[c, g] = miss at the LAST index with
 *       fppi <= fppi_grid[g].  So a grid value below the first fppi gives 1, the last prediction holds up to +inf, and a class with
 *       labels and no predictions has a row of ones.  Counts are exact integers; each value is one division and one subtraction.
 *       This is the Caltech (Dollar et al.) false-positives-per-image / miss-rate curve on this evaluator's own matching; the
 *       log-average miss rate is the geometric mean of mr at np.logspace(-2, 0, 9), taken on the host.
 *   tp_bits, conf, pcls, n, label_hist, nc : as for cft_eval_ap;  n_images >= 1 : the images seen
 *   px [1000] : np.linspace(0, 1, 1000) (device)
 *   fppi_grid [ng] (device) and fppi_grid_host [ng] (the same values on the host, checked there): finite, non-decreasing,
 *       1 <= ng <= 4096
 * workspace: >= the bytes cft_eval_curves_workspace_bytes(n, nc, &bytes) gives, 256-byte aligned; the layout is cft_eval_ap's, so
 * a buffer sized for one call serves the other.  Its contents after the call are unspecified.  Every argument is checked before the
 * first launch (CFT_EINVAL, nothing launched).  No allocation, no synchronisation, no atomics: two calls give the same bits.
 */
int cft_eval_curves_workspace_bytes(long n, int nc, long* bytes);
int cft_eval_curves(const unsigned short* tp_bits, const float* conf, const int* pcls, long n, const int* label_hist, int nc, int n_images,
                    const double* px, const double* fppi_grid, const double* fppi_grid_host, int ng, void* workspace, long workspace_bytes,
                    double* pcurve, double* rcurve, double* f1curve, double* pycurve, double* mr, int* best, void* stream);

/*
 * cft_eval_confusion replaces ConfusionMatrix.process_batch (utils/metrics.py:119-157) as test.py:193-194 feeds it, for a whole
 * batch: the grouping launch of cft_eval_match, then one workgroup per image.  An image counts only if it has a label and an
 * NMS detection (test.py:140-143, :186).  Detections are kept if conf > conf_thres, classes are truncated toward zero (.int()),
 * the detection class is 0 with single_cls.  Pairs with box_iou > iou_thres (float32, utils/general.py:422-444) are candidates;
 * each detection keeps its highest-IoU label, then each label its highest-IoU detection among those that kept it (the two
 * argsort / np.unique passes of :138-141); exactly equal IoUs, which numpy's unstable argsort leaves open, go to the lowest
 * label index, then to the lowest detection row.  A matched label adds 1 at [detection class, label class], any other label at
 * [nc, label class], a kept detection in no match at [its class, nc] - the last only if the image has a match (`if n:`, :154).
 *   dets, counts, targets, img_h, img_w, geom : as for cft_eval_match
 *   native != 0  : dets and targets columns 2..5 are native-space xyxy already (process_batch's own arguments); geom unused
 *   matrix       : int64 [(nc + 1) * (nc + 1)], row = predicted class, column = true class, ACCUMULATED into (device)
 *   flag         : int [1] (device), bits OR-ed in: 1 = a label class outside [0, nc), 2 = a detection class outside [0, nc);
 *                  such labels / detections are not counted.  A matched label whose detection has a bad class is dropped
 *                  altogether (not counted as background), and its match still enables the image's leftover-detection pass
 * workspace: >= the size cft_eval_confusion_workspace_bytes stores in *bytes (host), 256-byte aligned.  Integer atomics only:
 * the result does not depend on scheduling.  No allocation, no synchronisation.
 */
int cft_eval_confusion_workspace_bytes(int B, int nt, int max_det, long* bytes);
int cft_eval_confusion(const float* dets, const int* counts, int B, int max_det, const float* targets, int nt, int img_h, int img_w,
                       const float* geom, float conf_thres, float iou_thres, int single_cls, int native, int nc, void* workspace,
                       long workspace_bytes, long long* matrix, int* flag, void* stream);

/*
 * cft_eval_export computes what test.py writes about each detection, float32, one rounding per operation in the reference's order:
 *   out [B, max_det, 16] : x1 y1 x2 y2 in native space (scale_coords, test.py:148-149) | conf, cls (0 with single_cls), valid (1 / 0), 0 |
 *                          xyxy2xywh / (w0, h0, w0, h0), the save_txt box (test.py:153-155) | left, top, w, h, the save_json box (:176-177)
 * Slots r >= counts[b] are zero.  out must be 16-byte aligned.  One launch, no allocation, no synchronisation.
 */
int cft_eval_export(const float* dets, const int* counts, int B, int max_det, const float* geom, int single_cls, float* out, void* stream);

/*
 * The device stage of detect_twostream.py between non_max_suppression and the files it writes (:129-153).  Both calls are
 * asynchronous, allocate nothing and do not synchronise.
 *
 * cft_detect_boxes computes what the loop says about each detection slot of the cft_nms output, float32 with one rounding per
 * operation in the reference's order.  out [B, max_det, 16], 32-bit words:
 *    0..3  x1 y1 x2 y2 (int)  scale_coords + clip_coords, then .round() (:131; half to even)
 *    4     cls (int)          int(cls), truncation toward zero (:147); -1 for a NaN
 *    5     conf (int)         hundredths 0..100, the digits of f'{conf:.2f}' (:148): correctly rounded, ties to even on the float's
 *                             exact binary value, computed in integers; values above 1 saturate at 100, negative ones and NaN give 0
 *    6     valid (int)        1 for r < counts[b]
 *    7     conf (float)       the confidence itself, what save_conf writes with %g (:142-144)
 *    8..11 x1 y1 x2 y2 (int)  the save_one_box rectangle (utils/general.py:628-637): xyxy2xywh of the rounded box, the larger side for
 *                             both when square != 0, wh * crop_gain + crop_pad, xywh2xyxy, .long() (toward zero), clip_coords;
 *                             the crop is rows [y1, y2) and columns [x1, x2)
 *    12..15 x y w h (float)   xyxy2xywh of the ROUNDED box / (w0, h0, w0, h0), the save_txt line (:141)
 * Slots r >= counts[b] are zero.  hist [B, nc] int (overwritten): detections per class of each image, the "3 persons, 1 car" line
 * (:134-136).  A class outside [0, nc) is not counted and ORs 1 into flag [1] (int, device).
 *   dets [B, max_det, 6] / counts [B] : the cft_nms output;  geom [B, 5] : h0, w0, gain, padw, padh as for cft_eval_match
 *   out must be 16-byte aligned; nc in [1, 32767]
 */
int cft_detect_boxes(const float* dets, const int* counts, int B, int max_det, const float* geom, int nc, float crop_gain, float crop_pad,
                     int square, int* out, int* hist, int* flag, void* stream);

/*
 * cft_detect_render draws the boxes of a whole batch into the device copies of the original images, both streams, in place, in one
 * launch (plot_one_box, utils/plots.py:67-81, as detect_twostream.py:139-151 calls it for reversed(det) on im0 and im0_).
 * cv2's anti-aliased thick lines and Hershey font are not reproduced ("parity with cv2 unpinned"); the raster is defined here.
 * For a valid slot with box (x1, y1, x2, y2), class c in [0, nc) and thickness t, all divisions integer, all ranges inclusive:
 *   outline     a = t / 2; the pixels of [x1 - a, x2 + a] x [y1 - a, y2 + a] that are not inside
 *               [x1 + t - a, x2 - t + a] x [y1 + t - a, y2 - t + a] take colour[c]; no anti-aliasing;
 *   label       (flag labels) the string is name[c], followed by ' ' and d.dd from the hundredths word when flag conf is set; n = its
 *               length, no label when n == 0; magnification m = max(1, (t + 1) / 3), glyph cell gw*m x gh*m;
 *     background columns x1 .. x1 + n*gw*m, rows y1 - gh*m - 3 .. y1 take colour[c] (the corners of utils/plots.py:79-80);
 *     text       character k occupies columns x1 + k*gw*m .. x1 + (k+1)*gw*m - 1, rows y1 - 1 - gh*m .. y1 - 2; pixel (px, py) of
 *                it takes the text colour where atlas[code - 32][(py - top) / m][(px - left) / m] >= 128 (a code outside 32..127
 *                draws as a space).
 * Everything is clipped to the h0 x w0 image (x2 == w0 is legal after clip_coords).  Painter's order is the reference's: it draws
 * reversed(det), outline, background, text, so a pixel ends as the covering slot with the LOWEST row index says, and within that
 * slot text wins over background over outline.  The kernel finds exactly that per pixel; each covered pixel is written once, by one
 * thread, uncovered pixels are neither read nor written: the image does not depend on scheduling.
 *   desc_dev / desc_host : B rows of cft_render_desc_t, device copy (read by the kernel) and the same bytes on the host (read by the
 *                          guards: pointers, strides, sizes are checked before the launch; nothing is launched on CFT_EINVAL).
 *                          img_ir may be NULL (one stream only)
 *   boxes [B, max_det, 16]: the cft_detect_boxes output (words 0..6 are read)
 *   colors [nc, 3] uint8 in the images' channel order; text_color = c0 | c1 << 8 | c2 << 16
 *   names [nc, name_ld] uint8 character codes, name_len [nc] int (clamped to [0, name_ld]); name_ld in [1, 32]
 *   atlas [96, gh, gw] uint8 for the codes 32..127; gh, gw in [1, 64]; thickness in [1, 64]
 * Two further flags serve plot_images (below); without them the output is what it was:
 *   CFT_RENDER_CONF1   (with flag conf) the suffix is ' ' and d.d from word 5 read as tenths 0..10 ('%.1f', utils/plots.py:185), four characters;
 *   CFT_RENDER_SIGNED  slot coordinates may be negative: they are clamped to [-2^24, 2^24] instead of [0, 2^24].  A box that starts left of
 *                      or above its image draws exactly the part inside: its off-image edge is not pulled to the border and its label starts
 *                      where the box starts.
 */
#define CFT_RENDER_DESC_BYTES 48
#define CFT_RENDER_LABELS 1
#define CFT_RENDER_CONF 2
#define CFT_RENDER_CONF1 4
#define CFT_RENDER_SIGNED 8
#define CFT_RENDER_MAX_NAME 32
typedef struct {
  unsigned char* img_rgb;         /* HWC uint8, pixels contiguous */
  unsigned char* img_ir;          /* same size, or NULL */
  long stride_rgb, stride_ir;     /* row strides in bytes, >= 3 * w0 */
  int h0, w0;
  int pad0, pad1;                 /* 0 */
} cft_render_desc_t;
int cft_detect_render(const void* desc_dev, const void* desc_host, int B, const int* boxes, int max_det, const unsigned char* colors, int nc,
                      int text_color, int thickness, int flags, const unsigned char* names, const int* name_len, int name_ld,
                      const unsigned char* atlas, int gh, int gw, void* stream);

/*
 * plot_images of the reference (utils/plots.py:128-203): the mosaic of the first batches that test.py / train.py save as
 * test_batch*_labels.jpg / _pred.jpg.  Five launches build it on the device: cft_mosaic_compose (the images into the grid),
 * cft_mosaic_slots (targets -> the slot table of cft_detect_render, which then draws every cell as one "image" with the flags
 * CFT_RENDER_CONF1 | CFT_RENDER_SIGNED), cft_mosaic_finish (file names and cell borders) and cft_mosaic_area (the final INTER_AREA
 * reduction).  All are asynchronous on the caller's stream, allocate nothing and do not synchronise; each pixel or slot is written by
 * one thread and only integer atomics are used: every result is the same run to run.  Arguments are checked on the host first;
 * nothing is launched on CFT_EINVAL.  cv2's float resize, anti-aliased lines and Hershey font are not reproduced ("parity with cv2
 * unpinned"); the raster below is this project's definition.
 *
 * Geometry (host, Python doubles, :142-152): bs = min(B, max_subplots), ns = ceil(sqrt(bs)), sf = max_size / max(H, W), with sf < 1
 * h = ceil(sf * H), w = ceil(sf * W), else h = H, w = W.  Cell i sits at block_x = w * (i / ns), block_y = h * (i % ns) (column-major).
 *
 * cft_mosaic_compose writes the HWC uint8 mosaic [ns*h, ns*w, 3] (row stride mstride bytes) of one stream from channels [c0, c0 + 3) of
 * the [B, C, H, W] batch img (dtype CFT_MOSAIC_U8 / F16 / F32; sb, sc, sh, sw = element strides, so a channel slice is a legal input).
 *   value   every element as float32, times 255 when the maximum of image 0 over all C channels is <= 1 (:137-138; the maximum is
 *           found on the device by a reduction launch in front, in maxkey [1] (device, 4 bytes, overwritten); a NaN counts as > 1),
 *           resized when resize != 0, clamped to [0, 255] (NaN: 0) and truncated toward zero;
 *   resize  float32 bilinear in OpenCV's published float convention: scale = 1 / (dst / src) in double, source coordinate
 *           f = (float)((d + 0.5) * scale - 0.5), s = floor(f), fraction a1 = f - s and a0 = 1 - a1 in float32, the indices s and s + 1
 *           clamped to the image (the fractions are kept); horizontal pass a0 * p0 + a1 * p1 on both rows, then vertical
 *           b0 * r0 + b1 * r1, every operation one float32 rounding (no fused multiply-add).  resize == 0 needs h == H and w == W;
 *   cells   without an image (i >= bs) are 255.
 *
 * cft_mosaic_slots fills slots [bs, cap, 16] int32 (words 0..3 x1 y1 x2 y2 relative to the cell, 4 cls, 5 tenths of the confidence,
 * 6 valid; the rest 0; 16-byte aligned), from one of two target forms:
 *   rows   [nt, cols] float32 (f64 == 0) or float64 (f64 != 0), cols 6 = image, class, x, y, w, h (labels) or 7 = the same and conf;
 *          a row belongs to image i when its first value equals i exactly; rows of other images are ignored;
 *   dets   (rows NULL) [B, max_det, 6] float32 xyxy conf cls with counts [B], the cft_nms output: output_to_target (:119-125) fused in,
 *          xyxy2xywh in float32, then the row treatment in float64.
 * Per image, in the rows' dtype with one rounding per operation (:166-179): xywh2xyxy; if the image has boxes and the maximum over
 * the four coordinates of all its boxes is <= 1.01 (the constant rounded to the dtype; a NaN is not), x * w and y * h; otherwise, if
 * *sf < 1, every coordinate * sf (sf: HOST double, rounded to the dtype); then int(), truncation toward zero.  Labels are always drawn, rows
 * with a confidence only if conf > 0.25.  The drawn targets of an image fill its slots in REVERSE order (the reference draws target j
 * after j - 1, cft_detect_render puts the lowest slot on top).  Word 5 = the digits of '%.1f' % conf: tenths 0..10, correctly rounded,
 * ties to even on the exact binary value, in integers (above 1: 10; negative or NaN: 0).  A class (truncated toward zero) outside [0, nc)
 * is skipped and ORs CFT_MOSAIC_BAD_CLASS into flag [1] (device int); more drawn targets than cap in one cell ORs CFT_MOSAIC_OVERFLOW
 * (the slots then hold the last cap drawn targets of that image).
 *
 * cft_mosaic_finish, after the boxes, one launch over both mosaics (img_ir may be NULL): the file name of cell i (codes [bs, 40]
 * uint8, name_len [bs] int clamped to [0, 40]; codes NULL: no text) from the glyph atlas with its top-left at (block_x + 5,
 * block_y + 5), magnification 1, colour (220, 220, 220) where the atlas value is >= 128, a code outside 32..127 as a space, clipped
 * to the cell; then the cell border of every occupied cell, white: the pixels of [block_x - 1, block_x + w + 1] x [block_y - 1,
 * block_y + h + 1] that are not inside [block_x + 2, block_x + w - 2] x [block_y + 2, block_y + h - 2] (the hard-edged form of
 * cv2.rectangle(..., thickness=3)), clipped to the mosaic.  Border over text over boxes.
 *
 * cft_mosaic_area: HWC uint8 3-channel INTER_AREA reduction [sh, sw] -> [dh, dw], the CFT_PAIR_AREA arithmetic bit for bit (equal
 * sizes: a copy); at most CFT_PAIR_MAX_REDUCTION per axis.  src and dst must not overlap.
 */
enum { CFT_MOSAIC_U8 = 0, CFT_MOSAIC_F16 = 1, CFT_MOSAIC_F32 = 2 };
#define CFT_MOSAIC_BAD_CLASS 1
#define CFT_MOSAIC_OVERFLOW 2
#define CFT_MOSAIC_NAME_CHARS 40
int cft_mosaic_compose(const void* img, int dtype, int B, int C, int H, int W, long sb, long sc, long sh, long sw, int c0, int bs, int ns,
                       int h, int w, int resize, unsigned char* mosaic, long mstride, int* maxkey, void* stream);
int cft_mosaic_slots(const void* rows, int nt, int cols, int f64, const float* dets, const int* counts, int B, int max_det, int bs, int cap,
                     int nc, int h, int w, const double* sf, int* slots, int* flag, void* stream);
int cft_mosaic_finish(unsigned char* img_rgb, unsigned char* img_ir, long stride_rgb, long stride_ir, int bs, int ns, int h, int w,
                      const unsigned char* codes, const int* name_len, const unsigned char* atlas, int gh, int gw, void* stream);
int cft_mosaic_area(const unsigned char* src, long src_stride, int sh, int sw, unsigned char* dst, long dst_stride, int dh, int dw,
                    void* stream);

/*
 * ComputeLoss of the reference (utils/loss.py:88-216) and its gradient with respect to the head outputs.
 *   p[l]      : host array of nl (1..5) device pointers, float32 contiguous [B, na, ny[l], nx[l], nc + 5] (Detect's raw list)
 *   ny, nx    : host arrays [nl]
 *   targets   : device float32 [nt, 6] = image, class, x, y, w, h (normalised); may be NULL when nt = 0
 *   anchors   : device float32 [nl, na, 2] in grid units (Detect.anchors)
 *   hyp       : HOST float64 [10] = box, obj, cls, cls_pw, obj_pw, anchor_t, fl_gamma, cp, cn, gr (cp / cn = smooth_BCE)
 *   balance   : device float64 [nl], read; with autobalance also updated as the reference does (ssi = stride-16 level)
 * cft_loss_forward writes loss [1] = (lbox + lobj + lcls) * B and items [4] = (lbox, lobj, lcls, loss) (device float32), and ORs
 * into err (device int): 1 = a target whose image index is outside [0, B) passed the anchor test, 2 = nc > 1 and a target whose
 * class is outside [0, nc) passed it.  Such targets are skipped (the reference raises on them).
 * build_targets' candidates are the reference's, in its order, compacted with prefix scans (capacity 5 * na * nt per level).
 * cft_loss_backward writes every element of grad[l] (host array of device pointers, shaped as p[l]) = d(loss * g) / dp[l],
 * g = grad_loss[0] (device); it reads what the last cft_loss_forward on the same workspace left there.
 * workspace: >= cft_loss_workspace_bytes(...) bytes, 256-byte aligned.  No allocation, no synchronisation, no float atomics.
 */
long cft_loss_workspace_bytes(int nl, int B, int na, const int* ny, const int* nx, int nc, int nt);
int cft_loss_forward(int nl, const float* const* p, int B, int na, const int* ny, const int* nx, int nc, const float* targets, int nt,
                     const float* anchors, const double* hyp, double* balance, int autobalance, int ssi, void* workspace,
                     long workspace_bytes, float* loss, float* items, int* err, void* stream);
/* byte offsets of the candidate lists in a forward's workspace: out[0] cell (int [nl][cap], ((b * na + a) * ny + gj) * nx + gi),
 * out[1] class (int [nl][cap]), out[2] tbox (float4 [nl][cap]), out[3] candidate counts (int [nl]); returns cap = 5 * na * nt */
long cft_loss_workspace_offsets(int nl, int B, int na, const int* ny, const int* nx, int nc, int nt, long* out);
int cft_loss_backward(int nl, const float* const* p, int B, int na, const int* ny, const int* nx, int nc, int nt, const float* anchors,
                      const double* hyp, const float* grad_loss, float* const* grad, void* workspace, long workspace_bytes,
                      void* stream);

/*
 * utils/autoanchor.py of the reference (check_anchors :23-59, kmean_anchors :103-201).  All three are asynchronous, allocate nothing
 * and use no float atomics; every result is the same run to run.  n < 2^24 labels, na <= 64 anchors, thr = 1 / anchor_t in [1/64, 1].
 *
 * cft_anchor_metric: x_ij = min over the two dims of min(r, 1 / r), r = wh_i / k_j (IEEE float32 divisions, bit-identical to torch on a
 * CPU), best_i = max_j x_ij.
 *   wh [n, 2], k [na, 2] float32 (device);  out: 8 x uint64 (device, overwritten):
 *   out[0] = sum_i [best_i > thr], out[1] = sum_ij [x_ij > thr], out[2] * 2^-29 + out[3] * 2^-61 = sum x, out[4] * 2^-29 + out[5] * 2^-61 =
 *   sum best (exact for terms >= 2^-38; smaller ones are cut below 2^-61), out[6] * 2^-29 = sum x[x > thr], out[7] * 2^-29 =
 *   sum best[best > thr], both exact.
 *
 * cft_anchor_kmeans: scipy.cluster.vq.kmeans(obs, k, iter=iters) in float64 (thresh 1e-5), one workgroup, the convergence test on the device.
 *   obs [n, 2] float64, whitened (device);  idx [iters, k] int (device): the rows each restart starts from (rng.choice(n, k, replace=False));
 *   book [k, 2] float64: the winning code book, its first info[0] rows;  dist [1] float64: its mean distance;
 *   info [4] int: surviving codes, winning restart, iterations over all restarts, 1 if a restart hit the iteration bound (100000).
 * workspace: >= the size cft_anchor_kmeans_workspace_bytes stores in *bytes (host), 256-byte aligned.
 *
 * cft_anchor_evolve: the genetic loop (:185-199), one launch per generation, the accept decision on the device.
 *   v [gen, na, 2] float64 (device): the mutations, drawn by the host;  k [na, 2] float64 (device): the anchors, updated in place;
 *   per generation kg = max(k * v, 2.0) in float64, fitness of float32(kg): fg = (float)((double)S / (2^29 * n)), S = the integer
 *   sum of best_i * 2^29 over best_i > thr; accepted when fg > f (float32, strict).
 *   f [1] float32: the fitness of k (written: first that of the incoming k);  flags [gen] int, fg [gen] float32: the trace.
 * workspace: >= the size cft_anchor_evolve_workspace_bytes stores in *bytes (host), 256-byte aligned.
 */
int cft_anchor_metric(const float* wh, long n, const float* k, int na, float thr, unsigned long long* out, void* stream);
int cft_anchor_kmeans_workspace_bytes(long n, long* bytes);
int cft_anchor_kmeans(const double* obs, long n, int k, const int* idx, int iters, void* workspace, long workspace_bytes, double* book,
                      double* dist, int* info, void* stream);
int cft_anchor_evolve_workspace_bytes(int gen, long* bytes);
int cft_anchor_evolve(const float* wh, long n, int na, float thr, const double* v, int gen, double* k, float* f, int* flags, float* fg,
                      void* workspace, long workspace_bytes, void* stream);

/*
 * The second half of a training step (train.py:560-563 `optim.SGD(..., nesterov=True)` + the two `add_param_group`s, :769
 * `scaler.step(optimizer)`, :773 `ema.update(model)`; utils/torch_utils.py:289-299 `ModelEMA.update`): ONE launch each over
 * every tensor, whatever their number.  fp32 only; plain loads and stores, no atomics, no LDS: every element is read and written by
 * exactly one thread, so the result is the same run to run.
 *
 * The tensors are described by a table that the caller builds once and keeps in device memory (`table_dev`, read by the kernel)
 * and, byte for byte, in host memory (`table_host`, read by the guards: every row is checked before the launch and nothing is
 * launched on CFT_EINVAL).  The table is nseg segment rows followed directly by nwork work rows:
 *   segment: one tensor.  n elements (may be 0); every pointer a multiple of 4.
 *   work   : cft_optim_work_t {seg, 0, start}: elements [start, min(start + chunk, n)) of segment seg.  The work rows list the
 *            chunks of segment 0 in order, then those of segment 1, ... (a segment of n elements has ceil(n / chunk) rows):
 *            the canonical cut, which the guards verify, so no element is covered twice.
 * chunk: elements per work row, a multiple of 1024 in [1024, 2^20] (CFT_OPTIM_CHUNK is what the Python side uses).  One workgroup
 * of 256 threads takes a work row at a time (grid-stride, at most max_blocks workgroups; 0 = CFT_OPTIM_MAX_BLOCKS).  A full chunk
 * whose pointers are all multiples of 16 moves as 16-byte words, anything else (tails, views at an odd storage offset) as dwords.
 *
 * cft_sgd_step: torch.optim.SGD with dampening = 0 and maximize = False.  hyper_host: HOST float [ngroups][4] = lr, momentum,
 * weight_decay, nesterov (0 / 1) of each param group, 1 <= ngroups <= CFT_OPTIM_MAX_GROUPS; it is copied into the kernel arguments
 * (changing it between calls costs no device copy).  grad_scale / found_inf: DEVICE float [1] each or NULL, as torch.amp.GradScaler
 * hands them to an optimizer with _step_supports_amp_scaling.  Per element, every a + s * b one fused multiply-add:
 *   g0 = grad_scale ? g * (float)(1.0 / (double)*grad_scale) : g
 *   g1 = wd != 0 ? fma(wd, p, g0) : g0
 *   b1 = momentum != 0 ? fma(momentum, b, g1) : g1          (b starts at zero: the first step gives b1 = g1, torch's clone)
 *   d  = nesterov ? fma(momentum, b1, g1) : b1
 *   p  <- fma(-lr, d, p);   b <- b1 when momentum != 0 (buf may be NULL in a group whose momentum is 0)
 * With found_inf given and *found_inf != 0 nothing is written.
 *
 * cft_ema_update: e <- fma(one_minus_d, m, d * e) over every segment (e = the EMA tensor, m = the model's); d and one_minus_d are
 * each computed in double by the caller and rounded to float, as `v *= d; v += (1. - d) * msd[k]` does with Python scalars.
 *
 * cft_adam_step: torch.optim.Adam / AdamW (train.py:558 `optim.Adam(pg0, lr=hyp['lr0'], betas=(hyp['momentum'], 0.999))`) with
 * amsgrad = False and maximize = False, on the same table layout (cft_adam_seg_t rows, then the canonical work rows) with the same
 * chunk / max_blocks / grad_scale / found_inf / stream arguments.  hyper_host: HOST double [ngroups][6] = lr, beta1, beta2, eps,
 * weight_decay, decoupled (0 = Adam's L2 term, 1 = AdamW's decay) of each param group; lr, eps, weight_decay >= 0, 0 <= beta < 1.
 * step: DEVICE float [1] per segment, the number of steps this tensor has taken; it stays on the device because only the device
 * knows whether found_inf skipped a step.  coef: DEVICE float [nseg][2] scratch, 8-byte aligned, written and read by this call only.
 * Two launches on the stream, the second reading what the first wrote:
 *   adam_prepare_kernel, one thread per segment: unless *found_inf != 0, s = *step + 1; *step = s; in double
 *     bc1 = 1 - pow(beta1, s), bc2 = 1 - pow(beta2, s); coef[seg] = {(float)(lr / bc1), (float)sqrt(bc2)} = {step_size, bc2_sqrt},
 *     what torch's single-tensor path computes with Python floats;
 *   adam_step_kernel, over the work rows as cft_sgd_step.  The float constants of a group are formed on the host from the doubles:
 *     w1 = (float)(1 - beta1), b2 = (float)beta2, w2 = (float)(1 - beta2), eps, wd, decay = (float)(1 - lr * wd).
 * Rounding rule, per element (floating-point contraction is off: an fma is where the rule says fma and nowhere else; sqrtf and /
 * are correctly rounded, the build has no fast-math flag):
 *   g0  = grad_scale ? g * (float)(1.0 / (double)*grad_scale) : g
 *   Adam  (L2), wd != 0:        g1 = fma(wd, p, g0);  p0 = p
 *   AdamW (decoupled), wd != 0: p0 = p * decay;       g1 = g0
 *   m1  = fma(w1, g1 - m, m)
 *   v1  = fma(w2 * g1, g1, b2 * v)
 *   den = sqrtf(v1) / bc2_sqrt + eps
 *   p  <- p0 + (-step_size * m1) / den;   m <- m1;   v <- v1
 * which is the order of operations of torch's single-tensor Adam (lerp_, mul_().addcmul_(), addcdiv_).  m and v start as zeros.
 * With found_inf given and *found_inf != 0 nothing is written, the step counters included.
 */
#define CFT_OPTIM_CHUNK 4096
#define CFT_OPTIM_MAX_BLOCKS 2048
#define CFT_OPTIM_MAX_GROUPS 8
#define CFT_SGD_SEG_BYTES 40
#define CFT_EMA_SEG_BYTES 24
#define CFT_ADAM_SEG_BYTES 56
#define CFT_OPTIM_WORK_BYTES 16
typedef struct { float* p; const float* g; float* buf; long n; long group; } cft_sgd_seg_t;
typedef struct { float* e; const float* m; long n; } cft_ema_seg_t;
typedef struct { float* p; const float* g; float* m; float* v; float* step; long n; long group; } cft_adam_seg_t;
typedef struct { int seg; int pad; long start; } cft_optim_work_t;
int cft_sgd_step(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                 const float* hyper_host, int ngroups, const float* grad_scale, const float* found_inf, void* stream);
int cft_ema_update(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                   float d, float one_minus_d, void* stream);
int cft_adam_step(const void* table_dev, const void* table_host, int nseg, long nwork, int chunk, int max_blocks,
                  const double* hyper_host, int ngroups, float* coef, const float* grad_scale, const float* found_inf, void* stream);

/*
 * Test-time augmentation of the single-stream model (reference models/yolo.py:113-128: scales 1 / 0.83 / 0.67, the middle view
 * mirrored left-right).  Two entry points, each one launch on the caller's stream; no allocation, no synchronisation, no atomics,
 * every output element written once: two runs give the same bits.  Every argument is checked on the host before the launch and
 * nothing is launched on CFT_EINVAL.
 *
 * cft_tta_view: scale_img (utils/torch_utils.py:247-257) of one view.  img is the [B, 3, H, W] batch, dtype CFT_TTA_U8 (each element
 * read as (float)u8 / 255.0f, IEEE division), CFT_TTA_F16 or CFT_TTA_F32; sb, sc, sh, sw = element strides, so channels [3, 6) of a
 * six-channel batch are a legal input.  ratio: host double in (0, 1]; gs >= 1 the grid size (the model's largest stride); flip 1 =
 * the image is mirrored left-right first.  With hs = (int)(H * ratio), ws = (int)(W * ratio) in doubles (Python's int()):
 *   resize  torch's bilinear with align_corners=False, every operation one float32 rounding, no fused multiply-add, per axis
 *             scale = (float)in / (float)out;  src = max(scale * (dst + 0.5f) - 0.5f, 0);  i0 = min((int)floorf(src), in - 1);
 *             i1 = min(i0 + 1, in - 1);  w1 = clamp(src - i0, 0, 1);  w0 = 1 - w1;
 *           value = (p00 * wx0 + p01 * wx1) * wy0 + (p10 * wx0 + p11 * wx1) * wy1;  a mirrored image reads column W - 1 - i;
 *   pad     rows >= hs and columns >= ws hold 0.447f, up to Ho = ceil(H * ratio / gs) * gs and Wo likewise (Python doubles);
 *   out     float32 [B, 3, Ho, Wo], contiguous, 16-byte aligned; Ho and Wo are checked against the formula.
 * The view of ratio 1 without a flip is the input itself (scale_img returns it); callers do not launch for it.
 *
 * cft_tta_merge: y0, y1, y2 = the views' float32 predictions [B, n_v, no] (contiguous) -> out [B, total, no], total = n0 + n1 + n2,
 * view after view along the row axis.  Columns 0..3 are divided by s_v (IEEE float32 division, what torch's CPU `/=` computes for
 * a Python scalar cast to float32); then column 0 of a view whose bit is set in flip_mask becomes img_w - x (one subtraction);
 * every other column is copied.  s_v in (0, 1]; no >= 5; no input may overlap out.
 */
enum { CFT_TTA_U8 = 0, CFT_TTA_F16 = 1, CFT_TTA_F32 = 2 };
int cft_tta_view(const void* img, int dtype, int B, int H, int W, long sb, long sc, long sh, long sw, const double* ratio, int gs,
                 int flip, float* out, int Ho, int Wo, void* stream);
int cft_tta_merge(const float* y0, const float* y1, const float* y2, int B, int n0, int n1, int n2, int no, float s0, float s1, float s2,
                  int flip_mask, float img_w, float* out, int total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFT_HIP_H */
