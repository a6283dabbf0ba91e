"""CPU-only checks of everything around the kernels: config generation, graph build, state-dict
compatibility, weight packing, BN folding, the C ABI surface, loud failure without a GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import msod_amd  # noqa: F401
from msod_amd import _lib, ops
from msod_amd.models import configs
from msod_amd.models.yolo_test import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm(d):
    d = dict(d)
    for part in ("backbone", "head"):
        d[part] = [[f, n, m, [None if a == "None" else a for a in args]] for f, n, m, args in d[part]]
    return d


def _reference_configs():
    """tests/golden/reference_configs.json (make_golden.py `configs`): hashes of the reference's model yamls as parsed, and the
    state-dict layout of the reference's own Model built from one of them."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as fh:
        return json.load(fh)


def _config_sha256(d):
    import hashlib
    import json
    return hashlib.sha256(json.dumps(d, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


@pytest.mark.parametrize("name", sorted(configs.REFERENCE_YAMLS))
def test_generated_config_equals_reference_yaml(name):
    assert _config_sha256(_norm(configs.named_config(name))) == _reference_configs()["yaml_sha256"][name]["normalised"]


def test_reference_yaml_file_builds_unchanged(tmp_path):
    """A yaml file whose parsed content is exactly the reference's (hash recorded from the reference file; Upsample's size
    written as the string 'None', as there) builds the network."""
    import yaml
    name = "yolov5s_fusion_transformerx3_vedai"
    d = configs.named_config(name)
    for part in ("backbone", "head"):
        d[part] = [[f, n, m, ["None" if a is None else a for a in args]] for f, n, m, args in d[part]]
    assert _config_sha256(d) == _reference_configs()["yaml_sha256"][name]["parsed"]
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(d, sort_keys=False))
    m = Model(str(path))
    assert m.yaml["nc"] == 9 and len(m.model) == 47


def test_graph_structure_flagship():
    m = Model(configs.named_config("cfg3"))
    assert len(m.model) == 47
    assert m.save == sorted(set(m.save)) or True
    assert [type(x).__name__ for x in m.model][:6] == ["Focus", "Conv", "C3", "Conv", "C3", "Focus"]
    assert m.model[5].f == -4                                   # IR stream entry
    assert sum(p.numel() for p in m.parameters()) == 206257992  # 206 M parameters
    gpts = [x for x in m.model if type(x).__name__ == "GPT"]
    assert [g.n_embd for g in gpts] == [256, 512, 1024]
    keys = set(m.state_dict())
    for k in ("model.0.conv.conv.weight", "model.0.conv.bn.running_var", "model.4.m.8.cv2.conv.weight",
              "model.10.pos_emb", "model.10.trans_blocks.7.sa.que_proj.bias", "model.10.trans_blocks.0.mlp.2.weight",
              "model.10.ln_f.weight", "model.46.m.2.bias", "model.46.anchors", "model.46.anchor_grid"):
        assert k in keys, k
    det = m.model[-1]
    assert torch.allclose(det.anchors[0], torch.tensor([[10., 13.], [16., 30.], [33., 23.]]) / 8)
    assert float(det.m[0].bias.view(3, -1)[0, 4]) != 0.0        # _initialize_biases ran


def test_derived_configs():
    c2 = configs.named_config("cfg2")
    assert sum(1 for r in c2["backbone"] if r[2] == "GPT") == 1
    m = Model(c2)
    assert abs(sum(p.numel() for p in m.parameters()) / 1e6 - 36.6) < 0.1
    c5 = configs.named_config("cfg5")
    assert (c5["depth_multiple"], c5["width_multiple"]) == (1.33, 1.25)
    assert [g.n_embd for g in Model(c5).model if type(g).__name__ == "GPT"] == [320, 640, 1280]


def test_fuse_matches_batchnorm_eval():
    torch.manual_seed(0)
    from msod_amd.models.common import Conv
    c = Conv(8, 16, 3, 1).eval()
    with torch.no_grad():
        c.bn.running_mean.normal_(0, 0.3); c.bn.running_var.uniform_(0.5, 2); c.bn.weight.uniform_(0.5, 1.5); c.bn.bias.normal_(0, 0.2)
    x = torch.randn(2, 8, 9, 9)
    want = c.bn(c.conv(x))
    w, b = ops.fold_bn(c.conv.weight, c.bn.weight, c.bn.bias, c.bn.running_mean, c.bn.running_var, c.bn.eps)
    assert c.bn.eps == 1e-3
    assert torch.allclose(F.conv2d(x, w, b, 1, 1), want, atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_conv_layout(dtype):
    """w[n][(kh*KW + kw)*cin_pad + ci], zero padded in ci, K and n."""
    w = torch.randn(10, 12, 3, 3)
    b = torch.randn(10)
    pk = ops.pack_conv(w, b, dtype, cin_pad=16)
    ge = 8 if dtype == torch.bfloat16 else 4
    assert pk.n == 16 and pk.cin == 16 and pk.kpad % (8 * ge) == 0 and pk.kpad >= 144 and pk.w.dtype == dtype
    full = pk.w.float()
    for (n, kh, kw, ci) in [(0, 0, 0, 0), (9, 2, 1, 11), (3, 1, 2, 5)]:
        assert full[n, (kh * 3 + kw) * 16 + ci] == w[n, ci, kh, kw].to(dtype).float()
    assert full[:, 144:].abs().max() == 0 and full[10:].abs().max() == 0
    assert full.view(16, -1)[:, :144].view(16, 9, 16)[:, :, 12:].abs().max() == 0
    assert torch.equal(pk.bias[:10], b) and pk.bias[10:].abs().max() == 0
    assert pk.flops_per_row == 2 * 10 * 9 * 12


def test_c_abi_exports_every_declared_symbol():
    """include/cft_hip.h is the only description of the ABI: _lib.SIGNATURES is parsed from it.  No prototype is skipped by the parser,
    the built library (loads without a GPU) exports every declared name and defines no ``cft_*`` symbol the header does not declare, and
    the parsed types of a few entry points equal the literal ones written out here."""
    import shutil
    import subprocess
    c = ctypes
    vp, i, l, f, ull = c.c_void_p, c.c_int, c.c_long, c.c_float, c.c_ulonglong
    header = open(os.path.join(ROOT, "include", "cft_hip.h")).read()
    stripped = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    declared = re.findall(r"\b(cft_\w+)\s*\(", stripped)
    assert len(declared) == len(set(declared)) == len(_lib.SIGNATURES) and set(declared) == set(_lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("cft_")}
        assert exported and exported <= set(declared), exported - set(declared)
    sig = {k: (r, list(a)) for k, (r, a) in _lib.SIGNATURES.items()}
    assert sig["cft_conv2d"] == (i, [vp] * 5 + [i] * 18 + [vp])
    assert sig["cft_attention"] == (i, [vp, vp, i, i, i, i, i, f, ull, vp])
    assert sig["cft_to_nhwc"] == (i, [vp, i, l, l, l, l, vp, i, i, i, i, i, i, i, i, vp])
    assert sig["cft_abi_version"] == (i, []) and sig["cft_last_error"] == (c.c_char_p, [])
    assert sorted(k for k, (r, _) in sig.items() if r is l) == [
        "cft_batchnorm_train_workspace", "cft_eval_ap_workspace_bytes", "cft_eval_match_workspace_bytes", "cft_loss_workspace_bytes",
        "cft_loss_workspace_offsets"]
    assert all(r is i for k, (r, _) in sig.items() if r is not l and k != "cft_last_error")
    macro = int(re.search(r"^#define\s+CFT_ABI_VERSION\s+(\d+)\s*$", header, re.M).group(1))
    lib = _lib.load()
    assert _lib.ABI_VERSION == lib.cft_abi_version() == macro
    assert lib.cft_abi_version.restype is i and lib.cft_loss_workspace_bytes.restype is l and lib.cft_conv2d.argtypes == sig["cft_conv2d"][1]
    assert (_lib.CFT_BF16, _lib.CFT_F32, _lib.CFT_F16, _lib.ACT_NONE, _lib.ACT_SILU, _lib.ACT_GELU) == (0, 1, 2, 0, 1, 2)


def test_header_parser_on_literal_snippets():
    """_lib.parse_header on the constructs include/cft_hip.h uses (and one it must refuse): multi-line prototypes, const qualifiers,
    unsigned long long, (void), commented-out prototypes, enumerators and the version macro; an unknown type raises, it is never
    defaulted to int."""
    c = ctypes
    sigs, consts = _lib.parse_header("""
        /* int cft_gone(int a); */
        // long cft_gone_too(void);
        #define CFT_ABI_VERSION 7
        enum { CFT_A = 0, CFT_B = -2 /* int cft_in_enum(int a); */ };
        int cft_probe(void);
        const char* cft_text(void);
        const char *cft_text2( void );
        long cft_many(const void* x, const float* const* pp, int n,   /* a comment, with commas, inside */
                      long stride, float eps,
                      unsigned long long seed, const int flag,
                      unsigned char* bytes, void* stream);
        int cft_none();
    """)
    assert consts == {"CFT_ABI_VERSION": 7, "CFT_A": 0, "CFT_B": -2}
    assert list(sigs) == ["cft_probe", "cft_text", "cft_text2", "cft_many", "cft_none"]
    assert sigs["cft_probe"] == (c.c_int, []) and sigs["cft_none"] == (c.c_int, [])
    assert sigs["cft_text"] == (c.c_char_p, []) and sigs["cft_text2"] == (c.c_char_p, [])
    assert sigs["cft_many"] == (c.c_long, [c.c_void_p, c.c_void_p, c.c_int, c.c_long, c.c_float, c.c_ulonglong, c.c_int, c.c_void_p, c.c_void_p])
    for bad, word in (("int cft_bad(double x);", "cft_bad"), ("int cft_bad2(int a, unsigned b);", "cft_bad2"), ("int cft_bad3(long long n);", "cft_bad3"),
                      ("int cft_bad4(size_t n);", "cft_bad4"), ("int cft_bad5(int);", "cft_bad5"), ("int cft_bad6(int a,);", "cft_bad6"),
                      ("double cft_bad7(int a);", "cft_bad7"), ("unsigned cft_bad8(void);", "cft_bad8")):
        with pytest.raises(ValueError, match=word + ":"):
            _lib.parse_header(bad)


def test_conv_variant_setter_knows_its_ids():
    """cft_set_conv_variant takes the ids of csrc/conv_gemm.hip's table (the forced tiles of test_gpu_ops.TILE_VARIANTS and the named
    CFT_CONV_* ids of the header) and no other: an unknown id returns -1, names itself in cft_last_error and leaves the setting as it
    was.  The setting is per host thread.  Nothing is launched: no GPU needed."""
    import threading
    from test_gpu_ops import TILE_VARIANTS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libcft_hip.so is not built")
    lib = _lib.load()
    named = [_lib._consts[k] for k in ("CFT_CONV_AUTO", "CFT_CONV_REGISTER_STAGED", "CFT_CONV_ASM", "CFT_CONV_ROUND5", "CFT_CONV_GENERIC_WALK")]
    assert named == [0, 1, 96, 97, 900] and _lib._consts["CFT_CONV_ASM_TILE"] == 960
    known = sorted(set(TILE_VARIANTS) | set(named) | {_lib._consts["CFT_CONV_ASM_TILE"] + t for t in (1, 2, 3, 4)})
    assert lib.cft_set_conv_variant(0) >= 0
    try:
        prev = 0
        for v in known:                                   # every known id round-trips: the next call returns it as the previous value
            assert lib.cft_set_conv_variant(v) == prev, v
            prev = v
        assert lib.cft_set_conv_variant(27) == prev
        for bad in (5, 91, 9201):
            assert lib.cft_set_conv_variant(bad) == -1
            assert str(bad).encode() in lib.cft_last_error()
            assert lib.cft_set_conv_variant(27) == 27     # the previous value stayed in force
        seen = []

        def other():
            seen.append(lib.cft_set_conv_variant(51))     # a fresh thread starts at the automatic choice
            seen.append(lib.cft_set_conv_variant(0))

        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen == [0, 51]
        assert lib.cft_set_conv_variant(0) == 27          # ... and its 51 never showed here
    finally:
        lib.cft_set_conv_variant(0)


class _OnGpu(torch.Tensor):
    """A meta tensor that says it lives on the GPU: the tensor forms of the eligibility predicates refuse anything else, and they only
    read its shape, strides and dtype."""
    is_cuda = True


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_chain_predicates_tensor_and_geometry_forms_agree(dtype):
    """ops.conv2d_chain_ok / conv2d_chain_res_ok (tensor) are adapters of their ``_geometry`` forms: the same answers for dense NHWC
    inputs, channel slices of a wider buffer (ldx, up to the launcher's 2^31-element limit on the buffer extent), a plain NCHW tensor
    (converted to dense first: ldx = cin), small and large pixel counts; anything that is not a 4-D GPU tensor of pk1.cin channels is
    refused by the tensor forms."""
    pk = lambda n, cin, k, s=1: ops.pack_conv(torch.zeros(n, cin, k, k), None, torch.bfloat16, s=s)      # noqa: E731
    pairs = [(pk(256, 256, 3), pk(256, 256, 1)), (pk(256, 128, 3, 2), pk(256, 256, 1)), (pk(128, 64, 3, 2), pk(128, 128, 1)),
             (pk(256, 256, 3), pk(512, 256, 1)), (pk(256, 256, 3), pk(256, 256, 3))]
    seen = set()
    for pk1, pk2 in pairs:
        for B, H, W, ld in ((64, 40, 40, None), (8, 40, 40, None), (31, 40, 40, None), (32, 40, 40, 512), (2, 9, 7, None),
                            (64, 640, 640, None), (64, 640, 640, 2 * pk1.cin), (1, 193, 256, 320)):
            x = torch.empty((B, H, W, ld or pk1.cin), dtype=dtype, device="meta").permute(0, 3, 1, 2)[:, :pk1.cin].as_subclass(_OnGpu)
            want = ops.conv2d_chain_ok_geometry(B, H, W, dtype, pk1, pk2, ldx=ld)
            assert ops.conv2d_chain_ok(x, pk1, pk2) is want
            for any_size in (False, True):
                want_res = ops.conv2d_chain_res_ok_geometry(B, H, W, dtype, pk1, pk2, any_size=any_size, ldx=ld)
                assert ops.conv2d_chain_res_ok(x, pk1, pk2, any_size=any_size) is want_res
                seen.add((want, want_res))
                Ho, Wo = ops.conv_out_size(H, W, pk1.k, pk1.s)
                assert want_res == (want and pk1.n == 256 and (any_size or B * Ho * Wo >= ops.CHAIN_RES_MIN_ROWS))
        nchw = torch.empty((4, pk1.cin, 40, 40), dtype=dtype, device="meta").as_subclass(_OnGpu)
        assert ops.conv2d_chain_ok(nchw, pk1, pk2) is ops.conv2d_chain_ok_geometry(4, 40, 40, dtype, pk1, pk2)
        assert ops.conv2d_chain_res_ok(nchw, pk1, pk2, any_size=True) is ops.conv2d_chain_res_ok_geometry(4, 40, 40, dtype, pk1, pk2, any_size=True)
        for not_x in (torch.empty((4, pk1.cin, 40, 40), dtype=dtype), torch.empty((4, pk1.cin + 8, 40, 40), dtype=dtype, device="meta").as_subclass(_OnGpu),
                      torch.empty((pk1.cin, 40, 40), dtype=dtype, device="meta").as_subclass(_OnGpu), None):
            assert ops.conv2d_chain_ok(not_x, pk1, pk2) is False and ops.conv2d_chain_res_ok(not_x, pk1, pk2, any_size=True) is False
    assert seen == ({(False, False)} if dtype == torch.float32 else {(True, True), (True, False), (False, False)})
    assert ops.conv_out_size(640, 641, 3, 2) == (320, 321) and ops.conv_out_size(20, 20, 1, 1) == (20, 20) and ops.conv_out_size(9, 7, 5, 2) == (5, 4)


def test_conv2d_chain_eligibility_is_a_host_decision():
    """cft_conv2d_chain_ok (no GPU): the chained kernel takes a first layer of exactly 128 or 256 output channels on the uniform K walk
    (cin % 64 == 0, no K padding), 16-bit operands, and a pointwise second layer no wider than the first - the 64 -> 128 and 128 -> 256
    stride-2 convs + C3.cv1|cv2 of yolov5l (reference models/common.py:45-50, 141-143) and cv2[j] + cv1[j+1] of its 256-channel head
    C3s; not the 256 -> 512 pair, yolov5x's 80 / 160-channel layers, fp32, or a padded K.  An ineligible pair is refused by the launcher."""
    lib = _lib.load()
    BF16, F32, F16 = 0, 1, 2
    ok_ = lib.cft_conv2d_chain_ok

    def ok(B, H, W, cin, n1, kpad1, k, s_, n2, dt, ldx=None, ldy=None):
        return ok_(B, H, W, cin, ldx or cin, n1, kpad1, k, s_, n2, ldy or n2, dt)
    assert ok(64, 320, 320, 64, 128, 576, 3, 2, 128, BF16) == 1            # yaml rows 1-2 / 6-7
    assert ok(64, 160, 160, 128, 256, 1152, 3, 2, 256, F16) == 1           # rows 3-4 / 8-9
    assert ok(64, 40, 40, 256, 256, 2304, 3, 1, 256, BF16) == 1            # head C3: cv2[j] + cv1[j+1]
    assert ok(1, 9, 9, 64, 128, 64, 1, 1, 8, BF16) == 1                    # any size, 1x1 first layer, narrow second layer
    assert ok(64, 80, 80, 256, 512, 2304, 3, 2, 512, BF16) == 0            # 512 channels do not fit a tile
    assert ok(16, 640, 640, 80, 160, 720, 3, 2, 160, BF16) == 0            # yolov5x widths
    assert ok(64, 320, 320, 64, 128, 576, 3, 2, 128, F32) == 0             # 16-bit only
    assert ok(64, 320, 320, 64, 128, 640, 3, 2, 128, BF16) == 0            # padded K
    assert ok(64, 320, 320, 32, 128, 288, 3, 2, 128, BF16) == 0            # cin % 64
    assert ok(64, 320, 320, 64, 128, 576, 3, 2, 136, BF16) == 0            # second layer wider than the first
    assert ok(64, 320, 320, 64, 128, 576, 3, 2, 100, BF16) == 0            # n2 % 8
    assert ok(0, 320, 320, 64, 128, 576, 3, 2, 128, BF16) == 0 and ok(64, 320, 320, 64, 128, 576, 2, 2, 128, BF16) == 0
    # 'ok' is the launcher's own validation, incl. its 2^31-element limits on the BUFFER extents (ld, not channel count)
    assert ok(64, 640, 640, 64, 128, 576, 3, 2, 128, BF16) == 1            # 64 * 640 * 640 * 64 = 1.7e9 elements
    assert ok(64, 640, 640, 64, 128, 576, 3, 2, 128, BF16, ldx=128) == 0   # the same input as a slice of a 128-channel buffer: 3.4e9
    assert ok(64, 640, 640, 64, 128, 576, 3, 2, 128, BF16, ldy=1024) == 0  # output slice of a 1024-channel buffer: 6.7e9
    assert ok(64, 320, 320, 64, 128, 576, 3, 2, 128, BF16, ldy=120) == 0   # ldy must cover the second layer's width
    # null / ineligible arguments are refused before any launch
    st = lib.cft_conv2d_chain(None, None, None, None, None, None, 1, 8, 8, 64, 64, 0, 128, 576, 3, 2, 128, 128, 0, 1, BF16, None)
    assert st == -1 and b"null pointer" in lib.cft_last_error()
    st = lib.cft_conv2d_chain(4096, 4096, None, 4096, None, 4096, 1, 8, 8, 64, 64, 0, 512, 576, 3, 2, 128, 128, 0, 1, BF16, None)
    assert st == -1 and b"not eligible" in lib.cft_last_error()


def test_bad_arguments_return_error_codes_without_gpu():
    lib = _lib.load()
    st = lib.cft_conv2d(None, None, None, None, None, 1, 8, 8, 8, 8, 0, 8, 64, 1, 1, 8, 0, 0, 0, 0, 0, 0, 0, None)
    assert st == -1 and b"null pointer" in lib.cft_last_error()
    st = lib.cft_layernorm(1, 1, 1, 1, 4, 6, 1e-5, 0, None)     # C not a multiple of 4; rejected before any launch
    assert st == -1
    # fused Focus: only 32/48/64/80 output channels, weights packed [n][192], even pointer/strides
    st = lib.cft_focus_conv(16, 0, 3 * 64 * 64, 64 * 64, 64, 1.0, 16, 192, None, 16, 40, 0, 1, 64, 64, 40, 1, 0, None)
    assert st == -1 and b"n must be 32, 48, 64 or 80" in lib.cft_last_error()
    st = lib.cft_focus_conv(16, 0, 3 * 64 * 64, 64 * 64, 64, 1.0, 16, 160, None, 16, 64, 0, 1, 64, 64, 64, 1, 0, None)
    assert st == -1 and b"[n][192]" in lib.cft_last_error()
    st = lib.cft_focus_conv(17, 1, 3 * 64 * 64, 64 * 64, 64, 1.0 / 255, 16, 192, None, 16, 64, 0, 1, 64, 64, 64, 1, 0, None)
    assert st == -1 and b"pixel-pair" in lib.cft_last_error()
    # fused Bottleneck: 64 / 128 channels only, and never in place (it reads a halo of x)
    st = lib.cft_bottleneck(4096, 256, 0, 16, 256, None, 16, 2304, None, None, 1 << 20, 256, 0, 1, 8, 8, 256, 1, 0, None)
    assert st == -1 and b"64 and 128 channels" in lib.cft_last_error()
    st = lib.cft_bottleneck(4096, 64, 0, 16, 64, None, 16, 576, None, None, 4096, 64, 0, 1, 8, 8, 64, 1, 0, None)
    assert st == -1 and b"overlaps the input" in lib.cft_last_error()
    st = lib.cft_bottleneck(4096, 128, 0, 16, 64, None, 16, 576, None, None, 4096 + 64, 128, 0, 1, 8, 8, 64, 1, 0, None)
    assert st == -1 and b"overlaps" in lib.cft_last_error()       # slices of one buffer that share channels [32,64)
    st = lib.cft_bottleneck_pack_w2(16, 576, 64, 32, 0, None)     # stage images exist for the 128-channel kernel only
    assert st == -1 and b"128 channels" in lib.cft_last_error()


def test_no_cpu_fallback():
    m = Model(configs.named_config("cfg1"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    m.train()
    with pytest.raises(RuntimeError):
        m.model[1](torch.zeros(1, 32, 8, 8))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "multispectral-object-detection_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f


def test_reference_pickled_checkpoint_loads_into_hip_modules():
    """A checkpoint pickled by the REFERENCE code (whole nn.Module, ``.half()``, train.py:850-860; tests/golden/ref_ckpt_tiny.pt,
    make_golden.py `ckpt`) un-pickles into this package's classes once the module aliases are installed, with identical parameters."""
    import sys
    from msod_amd import compat
    ck = os.path.join(ROOT, "tests", "golden", "ref_ckpt_tiny.pt")
    model = compat.attempt_load(ck, map_location="cpu")
    assert type(model).__module__.startswith("msod_amd") and model.compute_dtype == torch.float32   # .float(), as the reference
    assert type(model.model[-1]).__name__ == "Detect" and not hasattr(model.model[1], "bn")     # fused
    assert all(p.dtype == torch.float32 for p in model.parameters())
    ups = [m for m in model.model if isinstance(m, torch.nn.Upsample)]
    assert len(ups) == 2 and all(type(u).__module__.startswith("msod_amd") for u in ups)
    raw = torch.load(ck, map_location="cpu", weights_only=False)["model"].float()                    # the same pickle, not fused
    unfused = Model(raw.yaml)
    unfused.load_state_dict(raw.state_dict())
    fused = unfused.fuse().state_dict()
    assert set(fused) == set(model.state_dict())
    assert all(torch.equal(fused[k], v) for k, v in model.state_dict().items())
    for name in ("models", "models.common", "models.yolo_test"):
        sys.modules.pop(name, None)


def test_stream_lanes_follow_the_ir_backbone():
    """Two-HIP-stream schedule: the IR backbone (everything downstream of an ``f == -4`` entry through
    single-input edges, plus Add2(index=1)) is lane 1; joins and the RGB backbone/head are lane 0."""
    m = Model(configs.named_config("cfg3"))
    lanes = m.stream_lanes()
    assert len(lanes) == 47
    assert [i for i, l in enumerate(lanes) if l == 1] == [5, 6, 7, 8, 9, 12, 15, 16, 19, 23, 24, 25, 28]
    for i, mod in enumerate(m.model):
        if type(mod).__name__ in ("GPT", "Add", "Concat", "Detect"):
            assert lanes[i] == 0
    add = Model(configs.named_config("cfg1")).stream_lanes()
    assert add[:10] == [0] * 10 and add[10:20] == [1] * 10 and set(add[20:]) == {0}


def test_concat_plan_routes_producers_into_concat_buffers():
    """Head Concats: Conv / Add sources write straight into their slice of the concat buffer (no copy);
    Upsample sources stay deferred copies.  Offsets follow the reference's torch.cat order (common.py:217-219)."""
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    m = Model(named_config("cfg3"))
    plan = m.concat_plan()
    concats = [i for i, l in enumerate(m.model) if type(l).__name__ == "Concat"]
    assert len(concats) == 4 and len(plan) == 6
    for prod, (cidx, off, c, total) in plan.items():
        srcs = [cidx + j if j < 0 else j for j in m.model[cidx].f]
        assert prod in srcs and type(m.model[prod]).__name__ in ("Conv", "Add", "C3")
        assert off == (0 if srcs.index(prod) == 0 else total - c) and 0 < c < total
    ups = [s for cidx in concats for s in (cidx + j if j < 0 else j for j in m.model[cidx].f) if type(m.model[s]).__name__ == "Upsample"]
    assert ups and not any(u in plan for u in ups)


def test_state_dict_layout_equals_the_reference_build():
    """The reference's own Model built from yolov5s_fusion_transformerx3_vedai.yaml has exactly this package's state-dict keys,
    in the same order, with the same shapes (layout recorded by make_golden.py `configs`), so reference checkpoints load as they are."""
    want = [(k, tuple(s)) for k, s in _reference_configs()["state_dict_layout_yolov5s_fusion_transformerx3_vedai"]]
    ours = Model(configs.named_config("yolov5s_fusion_transformerx3_vedai"))
    assert [(k, tuple(v.shape)) for k, v in ours.state_dict().items()] == want


def test_bench_parity_check_flags_a_wrong_batch():
    """bench.py's `parity_at_bench_shape`: green for outputs at the reference-style bf16 error level, red for a forward that is off
    (wrong weights / a broken kernel) and red for a bf16 result that is much worse than the reference's own bf16 - the run then exits 3."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    want = [torch.randn(4, 3, 8, 8, 8, generator=g), torch.randn(4, 3, 4, 4, 8, generator=g)]
    noise = lambda s: [w + s * torch.randn(w.shape, generator=g) for w in want]      # noqa: E731
    ref16 = [r[:2] for r in noise(0.02)]
    ok = bench.parity_at_bench_shape("bf16", noise(0.02), want, ref16, 2)
    assert ok["ok"] and ok["pairs"] == 4 and ok["vs_reference_style_bf16"]["ok"]
    assert "NOT the literal 1e-2" in ok["gate"] and ok["meets_north_star_bound"] is False      # bf16 says in words what it is gated on
    f16 = bench.parity_at_bench_shape("f16", noise(0.002), want)
    assert f16["meets_north_star_bound"] is True and "parity-green" in f16["gate"]
    assert not bench.parity_at_bench_shape("bf16", noise(0.5), want, ref16, 2)["ok"]             # absolute bound
    worse = bench.parity_at_bench_shape("bf16", noise(0.06), want, ref16, 2)                     # inside 2.5e-2? no - and 3x the reference level
    assert not worse["ok"]
    assert bench.parity_at_bench_shape("f16", noise(0.002), want)["ok"] and not bench.parity_at_bench_shape("f16", noise(0.1), want)["ok"]
    assert bench.parity_at_bench_shape("f32", noise(1e-5), want)["ok"] and not bench.parity_at_bench_shape("f32", noise(0.01), want)["ok"]


def test_bench_dump_outputs_budget_and_sample(tmp_path):
    """bench.py --dump-outputs: float32 .npy files of pred and the raw maps; a batch above the 64 MB budget keeps the same
    seeded subset of pairs in every array, identical from call to call; a batch within the budget is written whole."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    b = 40
    pred = torch.randn(b, 25200, 8, generator=g).bfloat16()
    raw = [torch.randn(b, 3, s, s, 8, generator=g).bfloat16() for s in (80, 40, 20)]
    a = bench.dump_outputs(str(tmp_path / "a"), pred, raw)
    again = bench.dump_outputs(str(tmp_path / "b"), pred, raw)
    assert a["rows"] == again["rows"] and a["rows"] == sorted(a["rows"]) and 0 < len(a["rows"]) < b
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["pred.npy", "raw0.npy", "raw1.npy", "raw2.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    rows = torch.tensor(a["rows"])
    for name, t in (("pred", pred), *((f"raw{i}", r) for i, r in enumerate(raw))):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, t[rows].float().numpy())
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{name}.npy"))
    small = bench.dump_outputs(str(tmp_path / "c"), pred[:2], [r[:2] for r in raw])
    assert small["rows"] == [0, 1] and np.array_equal(np.load(tmp_path / "c" / "pred.npy"), pred[:2].float().numpy())


def test_shader_clock_summary_arithmetic():
    """bench.py's reading of cft_clock_probe samples: MHz = shader ticks / wall ticks x wall-clock rate; the FMA rate against the idle probe."""
    import ctypes
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    pr = object.__new__(bench.ShaderClockProbe)          # no GPU: fill the fields the summary reads
    pr.khz = ctypes.c_int(100000)                        # 100 MHz wall clock
    pr.max = 4
    pr.buf = torch.tensor([[420000, 20000, 80000, 0],    # 200 us at 2100 MHz, 400 FMA/us
                           [400000, 20000, 76000, 0],    # 2000 MHz
                           [440000, 20000, 84000, 0],    # 2200 MHz
                           [0, 0, 0, 0],
                           [480000, 20000, 90000, 0]], dtype=torch.int64)
    pr.n = 4                                             # the fourth sample never ran (wall ticks 0): dropped
    pr.idle = pr.buf[4].tolist()
    s = pr.summary()
    assert s["samples"] == 3 and s["s_memtime_mhz"] == {"median": 2100.0, "min": 2000.0, "max": 2200.0}
    assert s["idle_gpu"]["s_memtime_mhz"] == 2400.0 and s["idle_gpu"]["dependent_fma_per_us"] == 450.0
    assert abs(s["fma_rate_vs_idle"] - 400.0 / 450.0) < 1e-3
    pr.n = 0
    assert pr.summary() is None


def test_cft_fusion_plan_and_nms_module_structure():
    """Host side of round 4's graph-level pieces (no GPU): ``Model.cft_fusion_plan`` finds the (Add2, Add2, Add) group behind every GPT
    block of an x3 config - the yaml rows reference models/transformer/yolov5l_fusion_transformerx3_FLIR_aligned.yaml wires as
    [4,10]/[9,10] -> 29, [14,17]/[16,17] -> 30, [22,26]/[25,26] -> 31 - and nothing in a config without GPT blocks; ``Model.nms()``
    appends / removes the reference's NMS module (models/yolo_test.py:306-318) and ``autoshape()`` wraps the model."""
    from msod_amd.models.common import NMS, autoShape
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    m = Model(named_config("cfg3"))
    assert m.cft_fusion_plan() == {11: (10, 12, 29), 18: (17, 19, 30), 27: (26, 28, 31)}
    assert Model(named_config("cfg1")).cft_fusion_plan() == {}
    # the Conv layers handed un-run to the C3 behind them (yaml rows 1-2, 3-4, 13-14 of the RGB stream, 6-7, 8-9, 15-16 of the IR
    # stream); rows 20 / 23 feed SPP and the head's stride-2 convs feed Concat: not in the plan
    chain = m.chain_plan()
    assert chain == frozenset({1, 3, 6, 8, 13, 15}) and 1 in m.save      # (row 1 is "saved" by the reference's f = -4 book-keeping only)
    n = len(m.model)
    m.nms()
    assert len(m.model) == n + 1 and type(m.model[-1]) is NMS and m.model[-1].f == -1 and m.model[-1].i == n
    assert m.cft_fusion_plan() == {11: (10, 12, 29), 18: (17, 19, 30), 27: (26, 28, 31)}      # re-derived after the structural change
    m.nms()                                        # idempotent
    assert len(m.model) == n + 1
    m.nms(False)
    assert len(m.model) == n and type(m.model[-1]) is not NMS
    w = m.autoshape()
    assert isinstance(w, autoShape) and w.autoshape() is w and w.names == m.names and torch.equal(w.stride, m.stride)
    m._print_biases()


def test_prefix_segments_and_executor_switches():
    """Model.prefix_segments (the image-only prefix of each backbone that Model.depth_first runs sub-batch by sub-batch): a Focus fed by x or
    x2 followed by f == -1 Conv / C3 rows with exactly one reader, ending on a C3; every executor switch is a property whose setter drops
    the captured graphs."""
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    m = Model(named_config("cfg3"))
    assert m.prefix_segments() == [(0, 4), (5, 9)] and m.prefix_segments(3) == [(0, 2), (5, 7)] and m.prefix_segments(2) == []
    assert Model(named_config("cfg1")).prefix_segments() == [(0, 4), (10, 14)]            # add-fusion: row 4 is also read by the Add
    assert Model(named_config("yolov5l_fusion_transformer_FLIR")).prefix_segments() == [(0, 2), (3, 5)]   # 4-GPT layout: GPT after P2
    assert (m.depth_first, m.splitk, m.chain_convs, m.chain_pairs, m.fuse_cft_outputs, m.plan_concats) == (None, True, True, True, True, True)
    for name, value in (("depth_first", (8, None)), ("splitk", False), ("chain_convs", False), ("chain_pairs", False),
                        ("fuse_cft_outputs", False), ("plan_concats", False)):
        m._graphs["sentinel"] = object()
        setattr(m, name, value)
        assert getattr(m, name) == value and not m._graphs, name


# ---- C3 launch plans (C3.launch_plan): cfg3's twelve C3s --------------------------------------------------------------------------
C3_STRIDE = {2: 4, 7: 4, 4: 8, 9: 8, 14: 16, 16: 16, 22: 32, 25: 32, 35: 16, 39: 8, 42: 16, 45: 32}      # yaml row -> image pixels per cell


def _blocks(n):
    return tuple(("block", j) for j in range(n))


def _res_chain(n):
    return (("cv1", 0),) + tuple(("pair_res", j) for j in range(n - 1)) + (("cv2", n - 1),)


PAIRS3 = (("cv1", 0), ("pair", 0), ("pair", 1), ("cv2", 2))


def _c3_plans(model, B, Himg, Wimg, dtype, want=None):
    """{row: (front, split, steps)} of every C3 of cfg3 for a B x Himg x Wimg image batch; ``want``: a restatement to hold each against."""
    plans = {}
    for i, stride in C3_STRIDE.items():
        c3, front = model.model[i], (model.model[i - 1] if i - 1 in model.chain_plan() else None)
        H, W = Himg // stride, Wimg // stride                  # the grid cv1|cv2 sees; a front conv (3x3, stride 2) reads twice that
        k = 1 if front is None else front.conv.stride[0]
        plans[i] = tuple(c3.launch_plan(B, H * k, W * k, dtype, front))
        if want is not None:
            assert plans[i] == want(c3, front, B, H, W, dtype), i
    return plans


def _restated_plan(c3, front, B, H, W, dtype):
    """C3's launch rules restated independently of the planner: from the ``ops.*_geometry`` predicates on freshly packed weights (inference)."""
    pk = lambda conv: ops.pack_conv(*ops.fold_bn(conv.conv.weight, conv.bn.weight, conv.bn.bias, conv.bn.running_mean, conv.bn.running_var,   # noqa: E731
                                                 conv.bn.eps), dtype, s=conv.conv.stride[0])
    how = None
    if front is not None:
        both = ops.pack_conv(torch.cat([c3.cv1.conv.weight, c3.cv2.conv.weight]), torch.zeros(2 * c3.cv1.conv.out_channels), dtype)
        how = "chained" if ops.conv2d_chain_ok_geometry(B, 2 * H, 2 * W, dtype, pk(front), both) else "separate"
    n, c_, lowp = len(c3.m), c3.cv1.conv.out_channels, dtype in (torch.bfloat16, torch.float16)
    cv1, cv2 = [pk(b.cv1) for b in c3.m], [pk(b.cv2) for b in c3.m]
    steps = _blocks(n)
    if lowp and c_ not in (64, 128) and c3.chain and c3.chain_pairs:
        if all(b.add for b in c3.m):
            if all(ops.conv2d_chain_res_ok_geometry(B, H, W, dtype, cv2[j], cv1[j + 1]) for j in range(n - 1)):
                steps = _res_chain(n)
        else:
            can = [ops.conv2d_chain_ok_geometry(B, H, W, dtype, cv2[j], cv1[j + 1]) for j in range(n - 1)] + [False]
            steps = []
            for j in range(n):
                took = j > 0 and can[j - 1]
                steps += [("block", j)] if not (took or can[j]) else ([] if took else [("cv1", j)]) + [("pair" if can[j] else "cv2", j)]
            steps = tuple(steps)
    return (how, False, steps)


def test_c3_launch_plans_of_cfg3(monkeypatch):
    """C3.launch_plan on a CPU-resident cfg3, every C3 at the geometry it sees: the front conv chained at 64 / 128 channels (rows 2, 7, 4, 9)
    and run separately in front of the 512-wide pairs (14, 16); 64 / 128-channel Bottlenecks left to their own forward (the patch-resident
    kernel); the shortcut chain in the 256-channel backbone C3s only from ops.CHAIN_RES_MIN_ROWS pixels; the shortcut-free pair chains at
    256 channels (35, 42), nothing at 512 (22, 25, 45).  fp32 and training chain nothing; C3.chain / C3.chain_pairs switch the pair forms off
    and leave the front chains alone."""
    from msod_amd.models.common import C3
    model = Model(configs.named_config("cfg3"))
    assert sorted(i for i, m in enumerate(model.model) if isinstance(m, C3)) == sorted(C3_STRIDE)
    bf16 = torch.bfloat16
    table = {2: ("chained", False, _blocks(3)), 7: ("chained", False, _blocks(3)), 4: ("chained", False, _blocks(9)), 9: ("chained", False, _blocks(9)),
             14: ("separate", False, _res_chain(9)), 16: ("separate", False, _res_chain(9)),
             22: (None, False, _blocks(3)), 25: (None, False, _blocks(3)), 45: (None, False, _blocks(3)),
             35: (None, False, PAIRS3), 42: (None, False, PAIRS3), 39: (None, False, _blocks(3))}
    small = dict(table)
    small[14] = small[16] = ("separate", False, _blocks(9))              # 2 * 12 * 16 pixels: below the size heuristic
    assert _c3_plans(model, 64, 640, 640, bf16, _restated_plan) == table
    assert _c3_plans(model, 2, 192, 256, bf16, _restated_plan) == small
    monkeypatch.setattr(ops, "CHAIN_RES_MIN_ROWS", 0)
    assert _c3_plans(model, 2, 192, 256, bf16, _restated_plan) == table
    assert _c3_plans(model, 2, 192, 256, torch.float16, _restated_plan) == table
    no_pairs = {i: (front, False, _blocks(len(model.model[i].m))) for i, (front, _, _) in table.items()}      # the front chains stay
    for i, (front, split, steps) in _c3_plans(model, 64, 640, 640, torch.float32, _restated_plan).items():
        assert (front, split, steps) == ("separate" if i in (2, 7, 4, 9, 14, 16) else None, False, _blocks(len(model.model[i].m))), i
    monkeypatch.setattr(C3, "chain_pairs", False)                        # what bench.py --no-pair-chain does
    assert _c3_plans(model, 64, 640, 640, bf16, _restated_plan) == no_pairs
    monkeypatch.setattr(C3, "chain_pairs", True)
    model.chain_convs = False                                            # C3.chain on every instance (and no conv is handed over any more)
    assert _c3_plans(model, 64, 640, 640, bf16, _restated_plan) == no_pairs
    model.chain_convs = True
    model.chain_pairs = False
    assert _c3_plans(model, 64, 640, 640, bf16) == no_pairs
    model.chain_pairs = True
    assert _c3_plans(model, 64, 640, 640, bf16) == table
    model.train()
    for i, (front, split, steps) in _c3_plans(model, 64, 640, 640, bf16).items():
        assert (front, split, steps) == ("separate" if i in (2, 7, 4, 9, 14, 16) else None, True, _blocks(len(model.model[i].m))), i


def test_c3_launch_plan_cache(monkeypatch):
    """One cache per C3, keyed on everything the decision reads: a repeated request asks ``cft_conv2d_chain_ok`` nothing and returns the
    same plan; another CHAIN_RES_MIN_ROWS, chain, chain_pairs (instance or class), training, dtype, B or source ld is decided afresh;
    ``invalidate_packed`` drops the cache."""
    from msod_amd.models.common import C3, invalidate_packed
    model = Model(configs.named_config("cfg3"))
    c3, front = model.model[14], model.model[13]
    asked, real = [], ops.conv2d_chain_ok_geometry
    monkeypatch.setattr(ops, "conv2d_chain_ok_geometry", lambda *a, **k: asked.append(a[:3]) or real(*a, **k))

    def fresh(*args, **kw):
        """The request makes a new cache entry, and asks the library unless it is the training form."""
        n, entries = len(asked), len(c3.__dict__.get("_plan_cache", {}))
        plan = c3.launch_plan(*args, **kw)
        new, n1 = len(c3._plan_cache) - entries, len(asked)
        assert new == 1 or (new == 0 and n1 == n)
        assert c3.launch_plan(*args, **kw) is plan and len(asked) == n1 and len(c3._plan_cache) == entries + new
        return new == 1 and (n1 > n or plan.split), plan
    base = (64, 80, 80, torch.bfloat16, front)
    decided, plan = fresh(*base)
    assert decided and len(asked) == 1 + 8 and plan.steps == _res_chain(9)          # the front pair, then 8 Bottleneck pairs
    assert fresh(*base) == (False, plan)
    monkeypatch.setattr(ops, "CHAIN_RES_MIN_ROWS", 64 * 40 * 40 + 1)
    assert fresh(*base) == (True, plan._replace(steps=_blocks(9)))
    monkeypatch.setattr(ops, "CHAIN_RES_MIN_ROWS", 0)
    assert fresh(*base)[0] and fresh(64, 80, 80, torch.float32, front)[0] and fresh(8, 80, 80, torch.bfloat16, front)[0]
    assert fresh(64, 80, 80, torch.bfloat16, front, ld_in=512)[0] and fresh(64, 80, 80, torch.bfloat16, front, 256)[0]
    assert fresh(64, 40, 40, torch.bfloat16)[0]                                     # no conv handed over: the grid is cv1|cv2's own
    c3.chain = False
    assert fresh(*base) == (True, plan._replace(steps=_blocks(9)))
    c3.chain = True
    c3.chain_pairs = False
    assert fresh(*base) == (True, plan._replace(steps=_blocks(9)))
    del c3.chain_pairs
    monkeypatch.setattr(C3, "chain_pairs", False)
    assert c3.launch_plan(*base).steps == _blocks(9)                                # (the entry of the instance switch: the key holds the value)
    monkeypatch.setattr(C3, "chain_pairs", True)
    assert fresh(*base) == (False, plan)
    c3.train()
    assert fresh(*base) == (True, plan._replace(split=True, steps=_blocks(9)))
    c3.eval()
    for b in range(1, 20):                                                          # bounded
        c3.launch_plan(b, 40, 40, torch.bfloat16)
    assert len(c3._plan_cache) <= 17
    invalidate_packed(model)
    assert "_plan_cache" not in c3.__dict__ and fresh(*base) == (True, plan)


# ---- the CFT residual stream (_ResidualStream) -------------------------------------------------------------------------------------
def _traced_gpt(monkeypatch, rows, n_layer=1, p=0.1, train=False, splitk=True):
    """Names of the ops calls of one ``GPT(d_model=256, block_exp=4)`` forward on ``rows`` token rows; the kernels are replaced by recorders that
    return empty tensors which say they live on the GPU."""
    from msod_amd.models.common import GPT
    calls = []

    def gpu(*shape, dtype=torch.bfloat16):
        return torch.empty(shape, dtype=dtype, device="meta").as_subclass(_OnGpu)

    def linear(x, pk, act=ops.ACT_NONE, residual=None, out=None, out_dtype=None):
        assert (residual is None and out is None) or (residual is out and out.dtype == out_dtype == torch.float32)
        calls.append(f"linear{pk.n}" + ("+gelu" if act == ops.ACT_GELU else "") + ("+x" if out is not None else "") + (":f32" if out is None and out_dtype == torch.float32 else ""))
        return out if out is not None else gpu(x.shape[0], pk.n, dtype=out_dtype or x.dtype)

    def norm(name):
        def fn(x, *a):
            out_dtype = a[-2]
            calls.append(name + (f"[{a[0].shape[0]}]" if name == "layernorm_reduce" else "") + (":f32" if out_dtype == torch.float32 else ""))
            return gpu(*x.shape, dtype=out_dtype)
        return fn
    monkeypatch.setattr(ops, "gpt_tokenize", lambda rgb, ir, pos, grid: gpu(rgb.shape[0], 128, rgb.shape[1], dtype=torch.float32))
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "layernorm", norm("layernorm"))
    monkeypatch.setattr(ops, "layernorm_reduce", norm("layernorm_reduce"))
    monkeypatch.setattr(ops, "attention", lambda qkv, B, h, dk, dkp, pdrop, T: calls.append(f"attention(p={pdrop:g})") or gpu(qkv.shape[0], h * dkp))
    monkeypatch.setattr(ops, "linear_splitk", lambda x, pk, s: calls.append(f"linear_splitk{pk.n}[{s}]") or gpu(s, x.shape[0], pk.n, dtype=torch.float32))
    monkeypatch.setattr(ops, "dropout_", lambda x, p_: calls.append(f"dropout(p={p_:g})"))
    monkeypatch.setattr(ops, "add_rows_", lambda x, y: calls.append("add_rows"))
    gpt = GPT(256, h=8, block_exp=4, n_layer=n_layer, embd_pdrop=p, attn_pdrop=p, resid_pdrop=p).train(train)
    for blk in gpt.trans_blocks:
        blk.splitk = splitk
    B = rows // 128
    gpt((gpu(B, 256, 16, 16), gpu(B, 256, 16, 16)))
    return calls


def test_cft_residual_stream_call_sequences(monkeypatch):
    """One transformer block + ln_f (d = 256, block_exp 4; ops.splitk_choice: out_proj 1, fc2 4 at 1024 rows, see test_splitk_choice_rule):
    which GEMM form adds to the residual stream and which LayerNorm form follows it, in inference with and without split-K and in training
    with and without dropout; pending partial sums reach the next block's ln_input and, from the last block, ln_f."""
    head = ["layernorm", "linear768", "attention(p=0)", "linear256+x", "layernorm", "linear1024+gelu"]
    in_place = head + ["linear256+x", "layernorm:f32"]
    assert _traced_gpt(monkeypatch, 1024) == head + ["linear_splitk256[4]", "layernorm_reduce[4]:f32"]
    assert _traced_gpt(monkeypatch, 8192) == in_place
    assert _traced_gpt(monkeypatch, 1024, splitk=False) == in_place
    assert _traced_gpt(monkeypatch, 1024, train=True, p=0.0) == ["dropout(p=0)"] + in_place
    drop = ["linear256:f32", "dropout(p=0.1)", "add_rows"]
    assert _traced_gpt(monkeypatch, 1024, train=True) == (["dropout(p=0.1)", "layernorm", "linear768", "attention(p=0.1)"] + drop
                                                          + ["layernorm", "linear1024+gelu"] + drop + ["layernorm:f32"])
    assert _traced_gpt(monkeypatch, 1024, n_layer=2) == (head + ["linear_splitk256[4]", "layernorm_reduce[4]"] + head[1:]
                                                         + ["linear_splitk256[4]", "layernorm_reduce[4]:f32"])


def test_executor_plans_reproduce_the_recorded_ones_and_follow_the_layer_list():
    """tests/golden/exec/plans.json (make_exec_golden.py): lanes, concat plan, chain plan, CFT fusion plan and prefix segments of the four
    graph structures, plain and after ``nms()``, are reproduced exactly; the cached layer graph is rebuilt whenever ``model.model`` holds
    other layers - ``nms()``, ``nms(False)``, a slice - without anybody naming a cache."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_exec_golden as recipe
    with open(os.path.join(ROOT, "tests", "golden", "exec", "plans.json")) as fh:
        want = json.load(fh)
    assert sorted(want) == sorted(recipe.STRUCTURES)
    assert want[recipe.X4]["plain"]["cft"]["7"] == [6, 8, None]          # the 4-GPT layout's P2 group has no Add
    for name in recipe.STRUCTURES:
        m = Model(configs.named_config(name))
        plain = json.loads(json.dumps(recipe.plans(m)))
        assert plain == want[name]["plain"], name
        g0, n = m.layer_graph(), len(m.model)
        assert m.layer_graph() is g0                                     # cached while the layer list stands
        m.nms()
        assert m.layer_graph() is not g0 and len(m.stream_lanes()) == n + 1
        assert json.loads(json.dumps(recipe.plans(m))) == want[name]["nms"], name
        m.nms(False)
        assert len(m.stream_lanes()) == n and json.loads(json.dumps(recipe.plans(m))) == plain
        m.model = m.model[:n - 1]                                        # drop Detect: the plans describe the 'n - 1' layers that are left
        assert len(m.layer_graph().layers) == n - 1 and len(m.stream_lanes()) == n - 1
        assert m.concat_plan() == {int(k): tuple(v) for k, v in want[name]["plain"]["concat"].items()}
        assert m.chain_plan() == frozenset(want[name]["plain"]["chain"])


def test_splitk_choice_rule():
    """ops.splitk_choice (host decision, measured in profiles/r05_splitk_ab.md): split only GEMMs on the uniform K walk whose 256 x 256 tiles
    leave >= 3/4 of the chip idle, only up to SPLITK_MAX_ROWS token rows, to the smallest split that yields 128 workgroups with >= 4 K
    steps each."""
    import torch
    from msod_amd import ops
    pk = lambda n, k: ops.pack_conv(torch.zeros(n, k), None, torch.bfloat16)      # noqa: E731
    assert ops.splitk_choice(8192, pk(1024, 4096), torch.bfloat16) == 1          # 64 pairs: never
    assert ops.splitk_choice(2048, pk(1024, 4096), torch.bfloat16) == 1          # above SPLITK_MAX_ROWS
    assert ops.splitk_choice(1024, pk(1024, 4096), torch.bfloat16) == 8          # 16 tiles -> 128 workgroups of 8 K steps
    assert ops.splitk_choice(1024, pk(256, 1024), torch.bfloat16) == 4           # 4 K steps per split is the floor
    assert ops.splitk_choice(1024, pk(256, 256), torch.bfloat16) == 1            # 4 K steps in all
    assert ops.splitk_choice(1024, pk(4096, 1024), torch.bfloat16) == 1          # wide N: 64 tiles already
    assert ops.splitk_choice(1024, pk(1024, 1000), torch.bfloat16) == 1          # K not on the uniform walk (padded)
    assert ops.splitk_choice(512, pk(1024, 4096), torch.float32) == 8            # fp32: 32-wide K steps


@pytest.mark.parametrize("gen, inc", [("tools/gen_conv_asm.py", "multispectral-object-detection_amd/csrc/conv_gemm_asm.inc"),
                                      ("tools/gen_bneck_asm.py", "multispectral-object-detection_amd/csrc/probes/bottleneck_asm.inc")])
def test_committed_asm_text_is_what_its_generator_writes(gen, inc, tmp_path):
    """The hand-scheduled K loops are GENERATED text (csrc/*.inc, committed so that a build needs no generator run): the committed file must
    be byte-for-byte what the committed generator writes - an edit of one without the other fails here, not on the GPU."""
    import subprocess
    import sys
    out = tmp_path / "gen.inc"
    subprocess.run([sys.executable, os.path.join(ROOT, gen), str(out)], check=True, env={**os.environ, "CONV_ASM_PAD_NOPS": "0"})
    assert out.read_bytes() == open(os.path.join(ROOT, inc), "rb").read()


def test_asm_loop_text_invariants():
    """Structural invariants of one generated K step (tools/gen_conv_asm.py): 64 MFMAs, 24 fragment reads, AP + 4 LDS-DMA requests, exactly
    one barrier, and every accumulator register of the (MT0 / MT1) m-tiles written exactly twice per step (k halves 0 and 1)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_conv_asm", os.path.join(ROOT, "tools", "gen_conv_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    op = "v_mfma_f32_16x16x32_bf16"
    for (mt0, mt1) in g.TILES:
        ap = (16 * (mt0 + mt1) + 63) // 64                    # A passes of the tile (emit())
        for grp, mt in ((0, mt0), (1, mt1)):
            for masked in (False, True):
                for c in (0, 1):
                    lines = [ln for item in g.step(op, c, grp, masked, mt, ap) for ln in ([item] if isinstance(item, str) else item)]
                    mf = [ln for ln in lines if ln.startswith(op)]
                    assert len(mf) == 8 * mt, (mt, masked, grp)
                    accs = [ln.split()[1].rstrip(",") for ln in mf]
                    assert all(accs.count(a) == 2 for a in set(accs)) and len(set(accs)) == 4 * mt
                    assert sum(ln.startswith("ds_read_b128") for ln in lines) == 2 * (mt + 4)
                    assert sum(ln.startswith("s_barrier") for ln in lines) == 1
                    assert sum(ln.startswith("buffer_load_dwordx4") for ln in lines) == ap + 4
                    # the barrier sits between the two MFMA halves, behind a full wait
                    b = next(i for i, ln in enumerate(lines) if ln.startswith("s_barrier"))
                    assert lines[b - 1] == "s_waitcnt vmcnt(0) lgkmcnt(0)"
                    assert sum(ln.startswith(op) for ln in lines[:b]) == 4 * mt
