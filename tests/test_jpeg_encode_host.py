"""Host tests (no GPU) of the JPEG encoder's host half (cft_jpeg_layout / cft_jpeg_quality_tables / cft_jpeg_write_bound /
cft_jpeg_write in csrc/jpeg_encode.hip, utils/jpeg.py).  The yardstick is PIL's file, ``Image.fromarray(a).save(f, 'JPEG', quality=q,
subsampling=s)``, byte for byte, over the matrix of jpeg_enc_ref.matrix(): sizes (width x height) 1x1, 7x5, 8x8, 16x16, 17x33, 40x24,
36x20, 9x50, 41x3, 64x48; noise, gradient, mixed and saturated primaries; grey, 4:4:4, 4:2:2, 4:2:0; quality 1, 30, 75, 95, 100."""
import ctypes
import io

import numpy as np
import pytest

import jpeg_enc_ref as E

import msod_amd  # noqa: F401
from msod_amd import _lib
from msod_amd.utils import jpeg as J


def test_wiring():
    c = ctypes
    vp, i, l = c.c_void_p, c.c_int, c.c_long
    assert "jpeg_encode.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 19 == _lib.load().cft_abi_version()
    sig = {k: (r, list(a)) for k, (r, a) in _lib.SIGNATURES.items()}
    assert sig["cft_jpeg_layout"] == (i, [i, i, i, i, i, vp])
    assert sig["cft_jpeg_quality_tables"] == (i, [i, vp])
    assert sig["cft_jpeg_write_bound"] == (i, [vp, vp])
    assert sig["cft_jpeg_write"] == (i, [vp, vp, vp, vp, l, vp])
    assert sig["cft_jpeg_encode_coef"] == (i, [vp, vp, i, vp])
    assert J.SHORT_BUFFER == 2 and J.JPEG_ENC_DESC.itemsize == 96
    assert _lib.missing_symbols() == []                     # what build() asks before it trusts a library's timestamp


def test_matrix_is_the_issue_s_and_inside_the_decoder_s_subset():
    """800 cases, and cft_jpeg_entropy reads every PIL file of them: no case is refused, so nothing below is skipped."""
    cases = E.matrix()
    assert len(cases) == 10 * 4 * 4 * 5 == len({c[0] for c in cases})
    assert all(J.jpeg_info(blob) is not None for *_, blob in cases)
    prim = E.content("primaries", 20, 36, 1)
    assert set(np.unique(prim)) == {0, 255}


def test_restatement_through_the_writer_equals_pil_byte_for_byte():
    bad = []
    for name, src, layout, q, want in E.matrix():
        ncomp, hmax, vmax = E.SAMPLING[layout]
        info = J.jpeg_layout(src.shape[1], src.shape[0], ncomp, hmax, vmax)
        got = J.jpeg_write(E.coefficients(src, q, layout), E.quality_tables(q), info)
        if got != want:
            bad.append(name)
    assert not bad, f"{len(bad)} of {len(E.matrix())} files differ from PIL: {bad[:10]}"


def test_restatement_coefficients_equal_the_decoded_ones_in_real_blocks():
    """The device half's criterion, on the restatement: every real block equals cft_jpeg_entropy of PIL's file, every dummy block is 0."""
    import jpeg_ref as R
    for name, src, layout, q, blob in E.matrix()[::7]:
        info, want, qtab = R.entropy(blob)
        assert np.array_equal(qtab, np.where(np.arange(3)[:, None] < int(info["ncomp"]), E.quality_tables(q), 0)), name
        got = E.coefficients(src, q, layout)
        real = E.real_block_mask(info)
        assert np.array_equal(got.reshape(-1, 64)[real], want.reshape(-1, 64)[real]), name
        assert not got.reshape(-1, 64)[~real].any(), name


def test_writer_round_trip_through_the_decoder():
    """Independent of the restatement: cft_jpeg_entropy of PIL's file, handed to cft_jpeg_write, gives that file back."""
    import jpeg_ref as R
    bad, dummies = [], 0
    for name, src, layout, q, blob in E.matrix():
        info, coef, qtab = R.entropy(blob)
        if int(info["ncomp"]) == 3:
            assert np.array_equal(qtab[1], qtab[2])
        else:
            qtab = qtab.copy()
            qtab[1:] = 1                                              # rows of absent components are not read
        dummies += int((~E.real_block_mask(info)).sum())
        if J.jpeg_write(coef, np.ascontiguousarray(qtab), info) != blob:
            bad.append(name)
    assert not bad, f"{len(bad)} files are not reproduced: {bad[:10]}"
    assert dummies > 0


def test_quality_tables_equal_pil_s_dqt_for_every_quality():
    from PIL import Image
    arr = E.content("mixed", 16, 16, 3)
    for q in range(1, 101):
        with Image.open(io.BytesIO(E.pil_file(arr, "420", q))) as im:
            want = [np.array(im.quantization[0]), np.array(im.quantization[1])]
        zz = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
        got = J.jpeg_quality_tables(q)
        assert np.array_equal(got, E.quality_tables(q)), q
        assert np.array_equal(got[1], got[2])
        # the file's own tables through the decoder (natural order, whatever order PIL hands its copy out in)
        import jpeg_ref as R
        _, _, file_tabs = R.entropy(E.pil_file(arr, "420", q))
        assert np.array_equal(got, file_tabs), q
        for t in (0, 1):
            assert sorted(got[t].tolist()) == sorted(want[t].tolist()) and (np.array_equal(got[t], want[t]) or np.array_equal(got[t][zz], want[t])), q
    for q in (0, 101, -5):
        with pytest.raises(ValueError):
            J.jpeg_quality_tables(q)


def test_layout_equals_info_of_pil_s_file():
    seen = set()
    for name, src, layout, q, blob in E.matrix()[::5]:
        ncomp, hmax, vmax = E.SAMPLING[layout]
        info = J.jpeg_layout(src.shape[1], src.shape[0], ncomp, hmax, vmax)
        assert info == J.jpeg_info(blob) and info.tobytes() == J.jpeg_info(blob).tobytes(), name
        seen.add((ncomp, hmax, vmax))
    assert seen == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    for bad in ((0, 5, 3, 1, 1), (5, 0, 3, 1, 1), (J.MAX_SIDE + 1, 5, 3, 1, 1), (5, 5, 2, 1, 1), (5, 5, 4, 1, 1), (5, 5, 1, 2, 1), (5, 5, 3, 1, 2),
                (5, 5, 3, 4, 1), (5, 5, 3, 0, 0), (-3, 5, 1, 1, 1)):
        with pytest.raises(ValueError):
            J.jpeg_layout(*bad)
    assert _lib.load().cft_jpeg_layout(5, 5, 3, 1, 1, None) == J.EINVAL
    assert J.jpeg_layout(J.MAX_SIDE, 1, 3, 2, 2)["bw"][0] == 2 * (J.MAX_SIDE // 16)


def _guarded_write(coef, qtab, info, cap):
    """cft_jpeg_write into a buffer of ``cap`` bytes with canaries on both sides: (status, nbytes, the bytes, canaries intact)."""
    pad = 64
    buf = np.full(cap + 2 * pad, 0xA5, dtype=np.uint8)
    n = ctypes.c_long(-7)
    st = _lib.load().cft_jpeg_write(coef.ctypes.data, qtab.ctypes.data, info.ctypes.data, buf[pad:].ctypes.data, cap, ctypes.byref(n))
    intact = bool((buf[:pad] == 0xA5).all() and (buf[pad + cap:] == 0xA5).all())
    return st, n.value, buf[pad:pad + max(n.value, 0)].tobytes(), intact


def test_capacity_is_respected_with_canaries():
    lib = _lib.load()
    for name, src, layout, q, blob in E.matrix()[3::41]:
        ncomp, hmax, vmax = E.SAMPLING[layout]
        info = J.jpeg_layout(src.shape[1], src.shape[0], ncomp, hmax, vmax)
        coef, qtab = E.coefficients(src, q, layout), E.quality_tables(q)
        bound = J.jpeg_write_bound(info)
        st, n, got, intact = _guarded_write(coef, qtab, info, bound)
        assert st == J.OK and intact and n == len(blob) <= bound and got == blob, name
        st, n, got, intact = _guarded_write(coef, qtab, info, len(blob))
        assert st == J.OK and intact and got == blob, name
        for cap in (len(blob) - 1, len(blob) - 2, len(blob) - 3, len(blob) // 2, 700, 400, 21, 3, 1, 0):
            if 0 <= cap < len(blob):
                st, n, _, intact = _guarded_write(coef, qtab, info, cap)
                assert st == J.SHORT_BUFFER and n == 0 and intact, (name, cap)
    # the worst block the format allows stays under the bound: every AC coefficient 10 bits wide with the longest codes
    info = J.jpeg_layout(16, 16, 3, 2, 2)
    coef = np.full(int(info["ncoef"]), -1023, dtype=np.int16)
    coef[0::64] = np.where(np.arange(6) % 2 == 0, 1023, -1024)
    st, n, got, intact = _guarded_write(coef, E.quality_tables(100), info, J.jpeg_write_bound(info))
    assert st == J.OK and intact and 0 < n
    import jpeg_ref as R
    back = R.entropy(got)
    assert back is not None and np.array_equal(back[1], coef)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    info = J.jpeg_layout(36, 20, 3, 2, 2)
    coef = np.zeros(int(info["ncoef"]), dtype=np.int16)
    qtab = E.quality_tables(75)
    assert _guarded_write(coef, qtab, info, 4096)[0] == J.OK
    n = ctypes.c_long(0)
    out = np.zeros(4096, dtype=np.uint8)
    args = [coef.ctypes.data, qtab.ctypes.data, info.ctypes.data, out.ctypes.data, 4096, ctypes.byref(n)]
    for k in (0, 1, 2, 3, 5):
        a = list(args)
        a[k] = None
        assert lib.cft_jpeg_write(*a) == J.EINVAL, k
    assert lib.cft_jpeg_write(*(args[:4] + [-1, args[5]])) == J.EINVAL
    # tables: a zero, an entry above 8 bits, chroma rows that differ
    for spoil in (lambda q: q.__setitem__((0, 5), 0), lambda q: q.__setitem__((1, 63), 256), lambda q: q.__setitem__((2, 0), q[2, 0] + 1)):
        q = qtab.copy()
        spoil(q)
        st, nb, _, intact = _guarded_write(coef, q, info, 4096)
        assert st == J.EINVAL and nb == 0 and intact
    # an info struct nobody laid out: a field changed, a restart interval, another sampling
    for field, value in (("ncoef", int(info["ncoef"]) + 64), ("restart_interval", 1), ("vmax", 1), ("width", 0), ("bw", [9, 1, 1]), ("cw", [36, 36, 18])):
        bad = info.copy()
        bad[field] = value
        assert _guarded_write(coef, qtab, bad, 4096)[0] == J.EINVAL, field
        b = ctypes.c_long(5)
        assert lib.cft_jpeg_write_bound(bad.ctypes.data, ctypes.byref(b)) == J.EINVAL and b.value == -1, field
        with pytest.raises(ValueError):
            J.jpeg_write_bound(bad)
    b = ctypes.c_long(5)
    assert lib.cft_jpeg_write_bound(None, ctypes.byref(b)) == J.EINVAL and b.value == -1
    assert lib.cft_jpeg_write_bound(info.ctypes.data, None) == J.EINVAL
    assert J.jpeg_write_bound(J.jpeg_layout(J.MAX_SIDE, J.MAX_SIDE, 3, 1, 1)) > 2 ** 31      # why the bound is a long
    # coefficients baseline coding cannot hold: an AC value of 11 bits, a DC difference of 12 bits; the limits themselves are written
    for idx, value, status in ((1, 1024, J.UNSUPPORTED), (1, -1024, J.UNSUPPORTED), (1, 1023, J.OK), (0, 2048, J.UNSUPPORTED), (0, -2048, J.UNSUPPORTED),
                               (0, 2047, J.OK), (64 * 3 + 63, -32768, J.UNSUPPORTED)):
        c = coef.copy()
        c[idx] = value
        st, nb, _, intact = _guarded_write(c, qtab, info, 4096)
        assert st == status and intact and (nb > 0) == (status == J.OK), (idx, value)
    # garbage in dummy blocks (36 x 20 at 4:2:0 has a dummy column and a dummy row of luma) changes nothing
    clean = _guarded_write(coef, qtab, info, 4096)[2]
    c = coef.reshape(-1, 64).copy()
    c[~E.real_block_mask(info)] = -32768
    assert (~E.real_block_mask(info)).sum() == 6 + 3 and _guarded_write(c.reshape(-1), qtab, info, 4096)[2] == clean
    with pytest.raises(ValueError):
        J.jpeg_write(coef[:-1], qtab, info)
    with pytest.raises(ValueError):
        J.jpeg_write(coef, qtab.astype(np.int32), info)


def test_many_threads_write_side_by_side():
    from concurrent.futures import ThreadPoolExecutor
    cases = E.matrix()[-80:]

    def one(case):
        name, src, layout, q, blob = case
        ncomp, hmax, vmax = E.SAMPLING[layout]
        return J.jpeg_write(E.coefficients(src, q, layout), E.quality_tables(q), J.jpeg_layout(src.shape[1], src.shape[0], ncomp, hmax, vmax))
    with ThreadPoolExecutor(16) as pool:
        got = list(pool.map(one, cases * 3))
    assert got == [c[4] for c in cases * 3]


def test_default_save_is_quality_75_at_420():
    """What detect and the mosaics rely on: ``Image.save`` of an RGB array to a .jpg name without options."""
    from PIL import Image
    arr = E.content("mixed", 24, 40, 9)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG")
    assert buf.getvalue() == E.pil_file(arr, "420", 75)
    assert J.is_jpeg_name("a/b.JPG") and J.is_jpeg_name("x.jpeg") and not J.is_jpeg_name("x.png") and not J.is_jpeg_name("jpg")
