"""Host-side checks of GPT on anchor grids other than 8 x 8 (no GPU): the supported range and its error messages, parameter shapes and
state-dict keys, pickling, the C launchers' argument checks, and the gfx950 code objects of the new kernels (no scratch, no spills)."""
import os
import pickle
import re

import pytest
import torch

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multispectral-object-detection_amd", "csrc")


def test_out_of_range_grids_raise_naming_the_limit():
    from msod_amd import ops
    from msod_amd.models.common import GPT
    for grid in ((33, 32), (1, 1025), (0, 8), (8, 0)):
        with pytest.raises(NotImplementedError, match="1024"):
            GPT(64, n_layer=1, vert_anchors=grid[0], horz_anchors=grid[1]).check_supported()
        with pytest.raises(NotImplementedError, match="1024"):
            ops._grid(grid)
    x = torch.zeros(1, 64, 4, 4)
    with pytest.raises(NotImplementedError, match="1024"):             # before any device work
        GPT(64, n_layer=1, vert_anchors=64, horz_anchors=32)([x, x])
    with pytest.raises(NotImplementedError, match="256"):
        GPT(2304, h=8, n_layer=1, vert_anchors=4, horz_anchors=4).check_supported()     # head width 288
    with pytest.raises(NotImplementedError, match="2048"):
        GPT(2304, h=9, n_layer=0, vert_anchors=4, horz_anchors=4).check_supported()     # d_model above the de-tokeniser's LDS row
    for grid in ((1, 1), (5, 7), (16, 16), (32, 32), (1, 1024), (8, 8)):
        assert GPT(64, n_layer=1, vert_anchors=grid[0], horz_anchors=grid[1]).check_supported() == grid


def test_pos_emb_shape_and_state_dict_keys():
    from msod_amd.models.common import GPT
    keys8 = set(GPT(64, n_layer=2).state_dict())
    for va, ha in ((4, 4), (4, 8), (16, 16), (5, 7)):
        m = GPT(64, n_layer=2, vert_anchors=va, horz_anchors=ha)
        assert tuple(m.pos_emb.shape) == (1, 2 * va * ha, 64)
        assert set(m.state_dict()) == keys8


def test_anchor_grid_survives_pickle():
    from msod_amd.models.common import GPT
    m = GPT(64, n_layer=1, vert_anchors=16, horz_anchors=4)
    r = pickle.loads(pickle.dumps(m))
    assert (r.vert_anchors, r.horz_anchors) == (16, 4) and tuple(r.pos_emb.shape) == (1, 128, 64)
    assert r.check_supported() == (16, 4)


def test_grid_launchers_reject_bad_arguments():
    """The C entry points validate before touching the device (fake non-null pointers are never dereferenced)."""
    from msod_amd import _lib
    lib = _lib.load()
    p = 16
    assert lib.cft_attention_tokens(p, p, 1, 0, 8, 64, 64, _lib.CFT_BF16, 0.0, 0, None) != 0
    assert "T must be" in lib.cft_last_error().decode()
    assert lib.cft_attention_tokens(p, p, 1, 2049, 8, 64, 64, _lib.CFT_BF16, 0.0, 0, None) != 0
    assert lib.cft_attention_tokens(p, p, 1, 512, 8, 64, 288, _lib.CFT_BF16, 0.0, 0, None) != 0          # dkp > 256
    assert lib.cft_gpt_tokenize_grid(p, 64, 0, p, 64, 0, p, p, 1, 8, 8, 64, 33, 32, _lib.CFT_BF16, None) != 0
    assert lib.cft_gpt_upsample_add_grid(p, 0, None, 0, 0, p, 64, 0, 1, 8, 8, 64, 32, 33, _lib.CFT_BF16, None) != 0
    assert lib.cft_gpt_upsample_add2_grid(p, p, 64, 0, p, 64, 0, p, 64, 0, p, 64, 0, None, 0, 0, 1, 8, 8, 4096, 4, 4,
                                          _lib.CFT_F32, None) != 0                                         # C > 2048


def _kernel_meta(src, name_re):
    return {name: m for name, m in helpers.kernel_notes(src).items() if re.search(name_re, name)}


@pytest.mark.parametrize("src,pattern,n", [("attention_tokens.hip", "attention_tokens_kernel", 32),
                                           ("pointwise.hip", "gpt_(tokenize|upsample)_kernel", 18)])     # 8 x 8 and run-time grid
def test_grid_kernels_have_no_scratch_and_no_spills(src, pattern, n):
    meta = _kernel_meta(os.path.join(CSRC, src), pattern)
    assert len(meta) == n, sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 512, (name, m)


def test_token_grid_follows_the_tokens():
    """The de-tokenisers take the grid from the tokens GPT.forward produced when the caller does not name it: 128 tokens are 8 x 8 by
    default but 4 x 16 when GPT says so (the dual de-tokeniser behind a GPT must not read them as 8 x 8)."""
    from msod_amd import ops
    t = torch.zeros(2, 128, 64)
    assert ops.token_grid(t) == (8, 8)
    t.anchor_grid = (4, 16)
    assert ops.token_grid(t) == (4, 16) and ops.token_grid(t, (8, 8)) == (8, 8)
    assert not ops.gpt_dual_tokens_ok(t)             # CPU tensor: never eligible, whatever the grid
