"""Host tests (no GPU) of the JPEG decoder's host half (cft_jpeg_info / cft_jpeg_entropy in csrc/jpeg.hip, utils/jpeg.py): the library's
entropy decode followed by the numpy restatement tests/jpeg_ref.py must equal PIL's decode of the same bytes, byte for byte, over the
matrix of jpeg_ref.matrix(); files outside the subset are refused without a byte written outside the buffers."""
import ctypes
import io

import numpy as np
import pytest

import jpeg_ref as R

import msod_amd  # noqa: F401
from msod_amd import _lib
from msod_amd.utils import jpeg as J


def test_wiring():
    c = ctypes
    vp, i, l = c.c_void_p, c.c_int, c.c_long
    assert "jpeg.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 19 == _lib.load().cft_abi_version()
    sig = {k: (r, list(a)) for k, (r, a) in _lib.SIGNATURES.items()}
    assert sig["cft_jpeg_info"] == (i, [vp, l, vp])
    assert sig["cft_jpeg_entropy"] == (i, [vp, l, vp, vp, vp])
    assert sig["cft_jpeg_decode_u8"] == (i, [vp, vp, i, vp, l, vp])
    assert (J.OK, J.UNSUPPORTED, J.EINVAL) == (0, 1, -1)
    assert J.JPEG_INFO.itemsize == 128 and J.JPEG_DESC.itemsize == 96


def test_matrix_equals_pil_byte_for_byte():
    cases = R.matrix()
    assert len(cases) == len(R.SIZES) * len(R.CONTENTS) * len(R.LAYOUTS) * len(R.OPTIONS) * len(R.QUALITIES)
    bad = []
    for name, blob, want in cases:
        got = R.decode(blob)
        if got is None or got.shape != want.shape or not np.array_equal(got, want):
            bad.append(name)
    assert not bad, f"{len(bad)} of {len(cases)} files differ from PIL or were refused: {bad[:10]}"


def test_info_matches_pil():
    from PIL import Image
    seen = set()
    for name, blob, _ in R.matrix():
        info = J.jpeg_info(blob)
        with Image.open(io.BytesIO(blob)) as im:
            assert (int(info["width"]), int(info["height"])) == im.size, name
            assert int(info["ncomp"]) == im.layers == len(im.layer), name
            for c, (_, h, v, _) in enumerate(im.layer):
                assert (int(info["hs"][c]), int(info["vs"][c])) == (h, v), name
        hm, vm = int(info["hmax"]), int(info["vmax"])
        W, H = int(info["width"]), int(info["height"])
        assert (int(info["mcus_x"]), int(info["mcus_y"])) == (-(-W // (8 * hm)), -(-H // (8 * vm)))
        blocks = 0
        for c in range(int(info["ncomp"])):
            assert int(info["bw"][c]) == int(info["mcus_x"]) * int(info["hs"][c]) and int(info["bh"][c]) == int(info["mcus_y"]) * int(info["vs"][c])
            assert int(info["cw"][c]) == -(-W * int(info["hs"][c]) // hm) and int(info["ch"][c]) == -(-H * int(info["vs"][c]) // vm)
            blocks += int(info["bw"][c]) * int(info["bh"][c])
        assert int(info["ncoef"]) == int(info["plane_bytes"]) == 64 * blocks
        assert (int(info["restart_interval"]) > 0) == ("opt1" in name)
        seen.add((int(info["ncomp"]), hm, vm))
    assert seen == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}


def _guarded_entropy(blob, info):
    """cft_jpeg_entropy into buffers with canaries on both sides: (status, canaries intact)."""
    n, pad = int(info["ncoef"]), 64
    coef = np.full(n + 2 * pad, 0x5A5A, dtype=np.int16)
    qtab = np.full(192 + 2 * pad, 0xA5A5, dtype=np.uint16)
    a = np.frombuffer(blob, dtype=np.uint8)
    st = _lib.load().cft_jpeg_entropy(a.ctypes.data, a.size, coef[pad:].ctypes.data, qtab[pad:].ctypes.data, info.ctypes.data)
    intact = (coef[:pad] == 0x5A5A).all() and (coef[pad + n:] == 0x5A5A).all() and (qtab[:pad] == 0xA5A5).all() and (qtab[pad + 192:] == 0xA5A5).all()
    return st, bool(intact)


def test_files_outside_the_subset_are_refused():
    from PIL import Image
    arr = R.content("mixed", 24, 40, 5)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=85, progressive=True)
    progressive = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(buf, format="JPEG", quality=85)
    cmyk = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    png = buf.getvalue()
    refused = {"progressive": progressive, "cmyk": cmyk, "png": png,
               "4x4 at 4:2:0": R.encode(R.content("noise", 4, 4, 6), "420", 90), "8x3 at 4:2:0": R.encode(R.content("noise", 8, 3, 7), "420", 90),
               "one byte": b"\xff", "SOI alone": b"\xff\xd8"}
    lib = _lib.load()
    for name, blob in refused.items():
        assert J.jpeg_info(blob) is None and R.decode(blob) is None, name
        a = np.frombuffer(blob, dtype=np.uint8)
        info = np.zeros((), dtype=J.JPEG_INFO)
        assert lib.cft_jpeg_info(a.ctypes.data, a.size, info.ctypes.data) == J.UNSUPPORTED, name
    # the 4:4:4 and 4:2:2 forms of the two small sizes stay inside the subset (only a halved width of 2 is replicated by libjpeg)
    for hw in ((4, 4), (8, 3)):
        blob = R.encode(R.content("noise", *hw, 8), "444", 90)
        assert np.array_equal(R.decode(blob), R.pil_decode(blob))
    # a supported file cut inside its entropy data, and one that has lost its EOI: info is fine, the entropy decode refuses
    good = R.encode(arr, "420", 85)
    info = J.jpeg_info(good)
    for cut in (len(good) - 2, len(good) - 40, len(good) // 2 + len(good) // 4):
        blob = good[:cut]
        info_cut = J.jpeg_info(blob)
        assert info_cut is not None and info_cut == info
        st, intact = _guarded_entropy(blob, info_cut)
        assert st == J.UNSUPPORTED and intact, cut
    st, intact = _guarded_entropy(good, info)
    assert st == J.OK and intact
    # an info struct that belongs to another file, null pointers, no bytes
    other = J.jpeg_info(R.encode(arr[:16], "420", 85))
    st, intact = _guarded_entropy(good, other)
    assert st == J.EINVAL and intact
    a = np.frombuffer(good, dtype=np.uint8)
    assert lib.cft_jpeg_info(a.ctypes.data, 0, info.ctypes.data) == J.EINVAL
    assert lib.cft_jpeg_info(None, a.size, info.ctypes.data) == J.EINVAL and lib.cft_jpeg_info(a.ctypes.data, a.size, None) == J.EINVAL
    assert lib.cft_jpeg_entropy(a.ctypes.data, a.size, None, None, info.ctypes.data) == J.EINVAL


def test_entropy_layout_and_tables():
    """Coefficients are in natural order per block and the tables are the file's own: dequantised DC / 8 is the block mean of a flat image."""
    from PIL import Image
    flat = np.full((16, 16, 3), 200, dtype=np.uint8)
    blob = R.encode(flat, "gray", 100)
    info, coef, qtab = R.entropy(blob)
    with Image.open(io.BytesIO(blob)) as im:
        zz = np.array(im.quantization[0])                          # PIL hands the tables out in natural order since 8.3
    assert sorted(qtab[0].tolist()) == sorted(zz.tolist()) and (qtab[1:] == 0).all()
    blocks = coef.reshape(-1, 64)
    assert blocks.shape[0] == 4 and (blocks[:, 1:] == 0).all() and (blocks[:, 0] * qtab[0, 0] == (200 - 128) * 8).all()


def test_many_threads_decode_side_by_side():
    from concurrent.futures import ThreadPoolExecutor
    cases = R.matrix()[-96:]
    with ThreadPoolExecutor(16) as pool:
        got = list(pool.map(lambda c: R.decode(c[1]), cases * 4))
    for (name, _, want), g in zip(cases * 4, got):
        assert np.array_equal(g, want), name


@pytest.mark.parametrize("reserve", [0, 10 * 96 + 8])
def test_decode_plan_meets_the_guards_of_decode_u8(reserve):
    """The staging plan and the row filler give cft_jpeg_decode_u8 what its guards demand: 16-byte aligned, disjoint ranges inside the
    upload behind the reserved prefix, and planes that ascend from 0 in multiples of 16 without overlap up to the plane total."""
    picked = {}
    for name, blob, _ in R.matrix():
        size, _, layout, opt, q = name.split("-")
        if size in ("1x1", "64x64") and opt == "opt0" and q == "q75":
            picked.setdefault((size, layout), blob)
    assert len(picked) == 2 * len(R.LAYOUTS)
    infos = [J.jpeg_info(b) for b in picked.values()]
    infos[3:3] = [None]
    infos.append(None)
    plan = J.decode_plan(infos, reserve)
    live = [k for k, info in enumerate(infos) if info is not None]
    ranges = [(0, reserve)]
    for k, info in enumerate(infos):
        if info is None:
            assert plan.coef_off[k] is None and plan.qtab_off[k] is None and plan.plane_bytes[k] == 0
            continue
        ranges += [(plan.coef_off[k], plan.coef_off[k] + 2 * int(info["ncoef"])), (plan.qtab_off[k], plan.qtab_off[k] + J.QTAB_BYTES)]
        assert plan.plane_bytes[k] % 16 == 0 and plan.plane_bytes[k] >= int(info["plane_bytes"])
    assert all(lo % 16 == 0 and 0 <= lo <= hi <= plan.upload_bytes for lo, hi in ranges)
    ranges.sort()
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    assert plan.plane_total == sum(plan.plane_bytes)
    upload, dsts = 0x7F0000001000, [(0x7E0000000000 + 0x100000 * j, 3 * int(infos[k]["width"]) + 5 * j) for j, k in enumerate(live)]
    table = np.zeros(len(live), dtype=J.JPEG_DESC)
    assert J.fill_decode_rows(table, plan, infos, live, upload, dsts) == plan.plane_total
    end = 0
    for row, k in zip(table, live):
        assert int(row["plane_off"]) % 16 == 0 and int(row["plane_off"]) >= end
        end = int(row["plane_off"]) + int(infos[k]["plane_bytes"])
    assert end <= plan.plane_total and int(table[-1]["plane_off"]) + plan.plane_bytes[live[-1]] == plan.plane_total
    want = np.zeros(len(live), dtype=J.JPEG_DESC)
    for row, got, k, (dst, stride) in zip(want, table, live, dsts):
        J.fill_desc(row, infos[k], upload + plan.coef_off[k], upload + plan.qtab_off[k], dst, stride, int(got["plane_off"]))
    assert want.tobytes() == table.tobytes()


def test_dataset_switch():
    """``decode`` is an attribute set in the constructor body, 'pil' by default, switched by use_device_jpeg on a dataset or a loader."""
    from msod_amd.utils import datasets as D
    ds = D.LoadMultiModalImagesAndLabels.__new__(D.LoadMultiModalImagesAndLabels)
    ds.decode = 'pil'
    loader = D.PairLoader.__new__(D.PairLoader)
    loader.dataset = ds
    assert D.use_device_jpeg(ds) is ds and ds.decode == 'device'
    assert D.use_device_jpeg(loader, enabled=False) is loader and ds.decode == 'pil'
    D.use_device_jpeg(loader)
    assert ds.decode == 'device'
    with pytest.raises(TypeError):
        D.use_device_jpeg(object())
