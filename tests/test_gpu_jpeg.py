"""GPU tests of the JPEG decoder's device half (cft_jpeg_decode_u8 in csrc/jpeg.hip, utils/jpeg.py) and of the loaders with
``decode='device'`` (utils/datasets.py): everything is compared with PIL's decode of the same bytes, byte for byte."""
import contextlib
import io
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as AR
import jpeg_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset")
OPT = SimpleNamespace(single_cls=False)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_matrix_in_one_batch(dev):
    """Every file of the matrix - mixed sizes, samplings, restart intervals - in one table and one call; every third destination has a
    padded row stride whose padding must survive; a second run gives the same bytes; the device stage waits for nothing."""
    from msod_amd.utils import jpeg as J
    cases = R.matrix()
    blobs = [b for _, b, _ in cases]

    def destinations():
        backing, out = [], []
        for k, (_, _, want) in enumerate(cases):
            h, w = want.shape[:2]
            if k % 3 == 0:
                big = torch.full((h, w + 5, 3), 0xEE, dtype=torch.uint8, device=dev)
                backing.append(big)
                out.append(big[:, :w])
            else:
                backing.append(None)
                out.append(None)
        return backing, out

    runs = []
    for _ in range(2):
        backing, out = destinations()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = J.decode_jpeg_batch(blobs, dev, out=out)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        runs.append((backing, got))
    bad = []
    for k, (name, _, want) in enumerate(cases):
        a, b = runs[0][1][k], runs[1][1][k]
        assert a is not None and a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == want.shape, name
        if not np.array_equal(a.cpu().numpy(), want) or not torch.equal(a, b):
            bad.append(name)
        big = runs[0][0][k]
        if big is not None:
            assert a.data_ptr() == big.data_ptr() and (big[:, want.shape[1]:] == 0xEE).all(), name
    assert not bad, f"{len(bad)} of {len(cases)} files differ from PIL or between two runs: {bad[:10]}"


def test_unsupported_slots_are_none_and_guards_refuse(dev):
    from PIL import Image
    from msod_amd import _lib
    from msod_amd.utils import jpeg as J
    arr = R.content("mixed", 40, 56, 3)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=85, progressive=True)
    good = R.encode(arr, "420", 85)
    got = J.decode_jpeg_batch([buf.getvalue(), good, good[:len(good) // 2], b"\x89PNG\r\n"], dev)
    assert got[0] is None and got[2] is None and got[3] is None
    assert np.array_equal(got[1].cpu().numpy(), R.pil_decode(good))
    assert J.decode_jpeg_batch([b"no"], dev) == [None]
    # a table whose planes do not fit the workspace is refused before anything is launched
    info = J.jpeg_info(good)
    dst = torch.zeros((40, 56, 3), dtype=torch.uint8, device=dev)
    table = np.zeros(1, dtype=J.JPEG_DESC)
    J.fill_desc(table[0], info, dst.data_ptr(), dst.data_ptr(), dst.data_ptr(), 3 * 56, 0)
    host = torch.from_numpy(table.view(np.uint8).reshape(-1)).pin_memory()
    small = torch.zeros(int(info["plane_bytes"]) - 16, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="outside the workspace"):
        J.jpeg_decode_u8(host.to(dev), host, 1, small)
    assert _lib.load().cft_last_error().decode().startswith("cft_jpeg_decode_u8")
    torch.cuda.synchronize()
    assert (dst == 0).all()


@pytest.fixture(scope="module")
def jpeg_tree(tmp_path_factory):
    """The ten fixture pairs re-encoded: RGB as 4:2:0 quality 90, IR as grayscale; labels copied."""
    from PIL import Image
    root = tmp_path_factory.mktemp("jpeg_pairs")
    for stream in ("rgb", "ir"):
        os.makedirs(root / stream / "images")
        shutil.copytree(os.path.join(ROOT, stream, "labels"), root / stream / "labels")
        for name in sorted(os.listdir(os.path.join(ROOT, stream, "images"))):
            with Image.open(os.path.join(ROOT, stream, "images", name)) as im:
                if stream == "rgb":
                    im.convert("RGB").save(root / stream / "images" / (name[:-4] + ".jpg"), quality=90, subsampling=2)
                else:
                    im.convert("L").save(root / stream / "images" / (name[:-4] + ".jpg"), quality=90)
    return root


@contextlib.contextmanager
def counting_device_decodes():
    """Counts the calls of cft_jpeg_decode_u8 the loaders make and the files they hand it: ``[calls, files]``."""
    from msod_amd.utils import jpeg as J
    inner, seen = J.jpeg_decode_u8, [0, 0]

    def counted(table_dev, table_host, n, workspace):
        seen[0], seen[1] = seen[0] + 1, seen[1] + n
        return inner(table_dev, table_host, n, workspace)
    J.jpeg_decode_u8 = counted
    try:
        yield seen
    finally:
        J.jpeg_decode_u8 = inner


def _passes(root, device_decode, cache=False, n=1):
    from msod_amd.utils import datasets as D
    loader, ds = quiet(D.create_dataloader_rgb_ir, str(root / "rgb" / "images"), str(root / "ir" / "images"), 64, 4, 32, OPT, rect=True, pad=0.5,
                       workers=4, cache=cache)
    assert ds.decode == 'pil'
    if device_decode:
        assert D.use_device_jpeg(loader) is loader and ds.decode == 'device'
    return [[(img.clone(), t, p, s) for img, t, p, s in loader] for _ in range(n)], ds


def _assert_same_batches(got, want):
    assert len(got) == len(want) > 0
    for (img, t, p, s), (img0, t0, p0, s0) in zip(got, want):
        assert img.dtype == torch.uint8 and img.shape == img0.shape and torch.equal(img, img0)
        assert torch.equal(t, t0) and p == p0 and s == s0


def test_loader_with_device_decode_equals_pil(dev, jpeg_tree):
    (want,), ds0 = _passes(jpeg_tree, False)
    assert len(ds0) >= 8 and all(f.endswith(".jpg") for f in ds0.img_files_rgb + ds0.img_files_ir)
    with counting_device_decodes() as seen:
        (got,), _ = _passes(jpeg_tree, True)
    assert seen == [len(want), 2 * len(ds0)]                      # one call per batch, every file of every pair decoded on the device
    _assert_same_batches(got, want)
    with counting_device_decodes() as seen:
        (first, second), ds = _passes(jpeg_tree, True, cache='device', n=2)
    assert seen == [len(want), 2 * len(ds0)]                      # the second pass reads the cache
    assert all(t is not None and t.is_cuda for t in ds.imgs_rgb + ds.imgs_ir)
    _assert_same_batches(first, want)
    _assert_same_batches(second, want)
    # the cached originals are PIL's decode of the files
    from msod_amd.utils import datasets as D
    for i in (0, len(ds) - 1):
        for t, f in ((ds.imgs_rgb[i], ds.img_files_rgb[i]), (ds.imgs_ir[i], ds.img_files_ir[i])):
            assert np.array_equal(t.cpu().numpy(), D.decode_image(f))


@pytest.fixture(scope="module")
def mixed_tree(jpeg_tree, tmp_path_factory):
    """Among the JPEG pairs: one PNG pair, one progressive RGB JPEG, one RGB-JPEG / IR-PNG pair."""
    from PIL import Image
    root = tmp_path_factory.mktemp("mixed_pairs") / "mixed"
    shutil.copytree(jpeg_tree, root)
    names = sorted(n[:-4] for n in os.listdir(root / "rgb" / "images"))
    png_pair, progressive, half = names[0], names[1], names[2]
    for stream in ("rgb", "ir"):
        os.remove(root / stream / "images" / (png_pair + ".jpg"))
        shutil.copy(os.path.join(ROOT, stream, "images", png_pair + ".png"), root / stream / "images" / (png_pair + ".png"))
    with Image.open(os.path.join(ROOT, "rgb", "images", progressive + ".png")) as im:
        im.convert("RGB").save(root / "rgb" / "images" / (progressive + ".jpg"), quality=90, progressive=True)
    os.remove(root / "ir" / "images" / (half + ".jpg"))
    shutil.copy(os.path.join(ROOT, "ir", "images", half + ".png"), root / "ir" / "images" / (half + ".png"))
    return root


def test_mixed_folder_is_judged_per_file(dev, mixed_tree):
    root = mixed_tree
    (want,), ds0 = _passes(root, False)
    assert {os.path.splitext(f)[1] for f in ds0.img_files_rgb + ds0.img_files_ir} == {".jpg", ".png"}
    with counting_device_decodes() as seen:
        (got,), _ = _passes(root, True)
    assert seen[1] == 2 * len(ds0) - 4                            # all but the three PNG files and the progressive one
    _assert_same_batches(got, want)
    (first, second), _ = _passes(root, True, cache='device', n=2)
    _assert_same_batches(first, want)
    _assert_same_batches(second, want)


def test_mixed_folder_with_cache_images_opens_no_file_in_the_second_pass(dev, mixed_tree, monkeypatch):
    """``cache_images=True`` over the mixed folder: JPEG and PNG files of one batch go through one upload into the batch's own buffer,
    and once every original is cached a pass neither decodes, probes nor launches the device decoder."""
    from msod_amd.utils import datasets as D
    (want,), _ = _passes(mixed_tree, False)
    loader, ds = quiet(D.create_dataloader_rgb_ir, str(mixed_tree / "rgb" / "images"), str(mixed_tree / "ir" / "images"), 64, 4, 32, OPT, rect=True,
                       pad=0.5, workers=4, cache=True)
    D.use_device_jpeg(loader)
    with counting_device_decodes() as seen:
        first = [(img.clone(), t, p, s) for img, t, p, s in loader]
    assert seen == [len(want), 2 * len(ds) - 4] and all(t is not None and t.is_cuda for t in ds.imgs_rgb + ds.imgs_ir)

    def refuse(*a, **k):
        raise AssertionError("a pass over cached originals opened a file")
    monkeypatch.setattr(D, "decode_image", refuse)
    monkeypatch.setattr(D, "_probe_jpeg", refuse)
    monkeypatch.setattr(ds, "load_pair", refuse)
    with counting_device_decodes() as seen:
        second = [(img.clone(), t, p, s) for img, t, p, s in loader]
    assert seen == [0, 0]
    _assert_same_batches(first, want)
    _assert_same_batches(second, want)


def test_a_pass_without_device_jpegs_reserves_no_jpeg_staging(dev):
    """``decode='pil'`` over the PNG fixture: one pass leaves the JPEG staging of both slots unallocated and launches no device decode;
    nor does ``decode='device'`` there, where every file is judged and none qualifies."""
    from msod_amd.utils import datasets as D
    loader, ds = quiet(D.create_dataloader_rgb_ir, os.path.join(ROOT, "rgb", "images"), os.path.join(ROOT, "ir", "images"), 64, 4, 32, OPT, rect=True,
                       pad=0.5, workers=4)
    assert ds.decode == 'pil' and len(loader) >= 2                 # both slots are used
    want = None
    for decode in ('pil', 'device'):
        D.use_device_jpeg(loader, enabled=decode == 'device')
        with counting_device_decodes() as seen:
            got = [(img.clone(), t, p, s) for img, t, p, s in loader]
        assert seen == [0, 0]
        slots = loader._pipe.slots
        assert all(s.pinned is not None and s.staged is not None for s in slots), decode
        assert all(s.jpinned is None and s.jstaged is None for s in slots), decode
        want = want or got
        _assert_same_batches(got, want)
    assert set(ds.jpeg_infos.values()) == {None} and len(ds.jpeg_infos) == 2 * len(ds)


def test_training_batch_is_the_same_with_both_decoders(dev, jpeg_tree):
    from msod_amd.utils import datasets as D
    hyp = next(c for c in AR.load_cases()[1] if c["name"] == "b64")["hyp"]
    batches = []
    for device_decode in (False, True):
        loader, ds = quiet(D.create_train_dataloader_rgb_ir, str(jpeg_tree / "rgb" / "images"), str(jpeg_tree / "ir" / "images"), 64, 4, 32, OPT, hyp,
                           workers=4, seed=5)
        assert ds.decode == 'pil'
        if device_decode:
            D.use_device_jpeg(ds)
        with counting_device_decodes() as seen:
            img, t, p, s = next(iter(loader))
            batches.append((img.clone(), t, p, s))
        assert (seen[0] >= 1) == device_decode
    _assert_same_batches(batches[1:], batches[:1])
    assert tuple(batches[0][0].shape) == (4, 6, 64, 64)
