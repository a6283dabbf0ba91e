"""GPU tests of the JPEG encoder's device half (cft_jpeg_encode_coef in csrc/jpeg_encode.hip, utils/jpeg.py) and of the callers that
switch to it (detect(opt) with device_jpeg, evaluate(plots=True, device_jpeg=True), plot_images).  Equality is the criterion
throughout: coefficients against cft_jpeg_entropy of PIL's file, files against PIL's bytes."""
import contextlib
import io
import os
import re
import shutil
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_enc_ref as E
import jpeg_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "dataset")
CKPT = os.path.join(ROOT, "tests", "golden", "ref_ckpt_tiny.pt")
PAD = 0xEE


def _sources(dev):
    """The matrix's images on the device, every third one as a view into a wider buffer filled with PAD: (backing list, views)."""
    backing, views = [], []
    for k, (_, src, _, _, _) in enumerate(E.matrix()):
        t = torch.from_numpy(np.array(src)).to(dev)
        if k % 3 == 0:
            big = torch.full((t.shape[0] + 1, t.shape[1] + 5) + tuple(t.shape[2:]), PAD, dtype=torch.uint8, device=dev)
            big[:t.shape[0], :t.shape[1]] = t
            backing.append(big)
            views.append(big[:t.shape[0], :t.shape[1]])
        else:
            backing.append(None)
            views.append(t)
    return backing, views


def _encode_table(dev, cases, views):
    """One table for cases of mixed quality, layout and size: (table host tensor, table device tensor, coefficient tensor, offsets, infos,
    what must stay alive)."""
    from msod_amd.utils import jpeg as J
    qualities = sorted({c[3] for c in cases})
    tabs_host = torch.from_numpy(np.stack([J.jpeg_quality_tables(q) for q in qualities]).view(np.uint8).reshape(-1)).pin_memory()
    tabs_dev = tabs_host.to(dev)
    infos = [J.jpeg_layout(v.shape[1], v.shape[0], *E.SAMPLING[c[2]]) for c, v in zip(cases, views)]
    offsets = np.concatenate([[0], np.cumsum([int(i["ncoef"]) for i in infos])])
    coef = torch.full((int(offsets[-1]) + 64,), 0x5A5A, dtype=torch.int16, device=dev)
    table = np.zeros(len(cases), dtype=J.JPEG_ENC_DESC)
    for row, c, v, info, off in zip(table, cases, views, infos, offsets):
        qi = qualities.index(c[3])
        row["src"], row["coef"], row["src_stride"] = v.data_ptr(), coef.data_ptr() + 2 * int(off), max(v.stride(0), v.shape[1] * int(info["ncomp"]))
        row["qtab"], row["qtab_host"] = tabs_dev.data_ptr() + 384 * qi, tabs_host.data_ptr() + 384 * qi
        J.fill_geometry(row, info)
    host = torch.from_numpy(table.view(np.uint8).reshape(-1)).pin_memory()
    return host, host.to(dev), coef, offsets, infos, (tabs_host, tabs_dev, table)


@pytest.fixture(scope="module")
def decoded():
    """cft_jpeg_entropy of PIL's file for every case of the matrix, computed once: a list of int16 arrays."""
    out = []
    for name, _, _, _, blob in E.matrix():
        e = R.entropy(blob)
        assert e is not None, f"{name}: the matrix holds a file the decoder refuses"
        out.append(e[1])
    return out


def test_whole_matrix_in_one_call(dev, decoded):
    """All 800 cases - grey and colour, three samplings, five qualities, mixed sizes, padded views - as one table and ONE launch: every
    real block equals the decoder's reading of PIL's file, every dummy block is zero, the value past the last block and the padding of
    the sources survive, a second run gives the same bits, and the launch waits for nothing."""
    from msod_amd.utils import jpeg as J
    cases = E.matrix()
    backing, views = _sources(dev)
    host, table_dev, coef, offsets, infos, keep = _encode_table(dev, cases, views)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        J.jpeg_encode_coef(table_dev, host, len(cases))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    first = coef.cpu().numpy()
    coef[:-64].fill_(0x1111)                                          # every value of the layout is written again, the canary stays
    J.jpeg_encode_coef(table_dev, host, len(cases))
    assert np.array_equal(coef.cpu().numpy(), first)
    assert (first[-64:] == 0x5A5A).all()
    bad, dummies = [], 0
    for k, (name, src, layout, q, _) in enumerate(cases):
        got = first[offsets[k]:offsets[k + 1]].reshape(-1, 64)
        real = E.real_block_mask(infos[k])
        dummies += int((~real).sum())
        if not np.array_equal(got[real], decoded[k].reshape(-1, 64)[real]) or got[~real].any():
            bad.append(name)
        if backing[k] is not None:
            big = backing[k].cpu().numpy()
            h, w = src.shape[:2]
            assert (big[h:] == PAD).all() and (big[:, w:] == PAD).all() and np.array_equal(big[:h, :w], src), name
    assert not bad, f"{len(bad)} of {len(cases)} images differ from PIL's coefficients: {bad[:10]}"
    assert dummies > 0


def test_encode_jpeg_batch_equals_pil_byte_for_byte(dev):
    """The public call, per (layout, quality) group of the matrix - sizes and contents mixed, padded views among them; the device stage
    (encode_jpeg_start) runs without a synchronisation."""
    from msod_amd.utils import jpeg as J
    cases = E.matrix()
    _, views = _sources(dev)
    J.encode_jpeg_batch(views[:1])                                    # first use: nothing lazy is left for the guarded region
    bad = []
    for layout in E.LAYOUTS:
        for q in E.QUALITIES:
            idx = [k for k, c in enumerate(cases) if c[2] == layout and c[3] == q]
            imgs = [views[k] for k in idx]
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                job = J.encode_jpeg_start(imgs, q, "4:2:0" if layout == "gray" else f"4:{layout[1]}:{layout[2]}")
            finally:
                torch.cuda.set_sync_debug_mode("default")
            got = job.all_bytes()
            assert len(got) == len(idx) == 40 and all(isinstance(g, bytes) for g in got)
            bad += [cases[k][0] for k, g in zip(idx, got) if g != cases[k][4]]
    assert not bad, f"{len(bad)} files differ from PIL: {bad[:10]}"
    # PIL's integer names of the subsampling, a [h, w, 1] grey image, a non-contiguous view (made contiguous), defaults = Image.save's
    k = next(i for i, c in enumerate(cases) if c[0] == "40x24-mixed-422-q75")
    assert J.encode_jpeg_batch([views[k]], 75, 1) == [cases[k][4]]
    g = next(i for i, c in enumerate(cases) if c[0] == "17x33-noise-gray-q75")
    assert J.encode_jpeg_batch([views[g].unsqueeze(2)]) == [cases[g][4]]
    k = next(i for i, c in enumerate(cases) if c[0] == "36x20-noise-420-q75")
    turned = views[k].transpose(0, 1)
    assert not turned.is_contiguous()
    assert J.encode_jpeg_batch([turned]) == [E.pil_file(np.ascontiguousarray(np.array(cases[k][1]).transpose(1, 0, 2)), "420", 75)]
    for wrong in ([views[k].cpu()], [views[k].float()], [views[k][..., :2]], []):
        with pytest.raises(ValueError):
            J.encode_jpeg_batch(wrong)
    with pytest.raises(ValueError):
        J.encode_jpeg_batch([views[k]], subsampling="4:1:1")
    with pytest.raises(ValueError):
        J.encode_jpeg_batch([views[k]], quality=0)


def test_one_larger_image_many_workgroups(dev):
    """640 x 512 noise at 4:2:0, quality 75: 7680 blocks, 240 workgroups; beside it a 16 x 16 one, whose workgroups past its own three
    have nothing to do."""
    from msod_amd.utils import jpeg as J
    big = E.content("noise", 512, 640, 77)
    small = E.content("mixed", 16, 16, 78)
    got = J.encode_jpeg_batch([torch.from_numpy(big).to(dev), torch.from_numpy(small).to(dev)], 75, "4:2:0")
    assert got[0] == E.pil_file(big, "420", 75) and got[1] == E.pil_file(small, "420", 75)


def test_bad_table_row_is_refused_and_nothing_is_launched(dev):
    from msod_amd import _lib
    from msod_amd.utils import jpeg as J
    cases = [c for c in E.matrix() if c[0] in ("36x20-mixed-420-q75", "17x33-noise-gray-q30")]
    views = [torch.from_numpy(np.array(c[1])).to(dev) for c in cases]
    host, table_dev, coef, offsets, infos, keep = _encode_table(dev, cases, views)
    table = host.numpy().view(J.JPEG_ENC_DESC)
    good = table.copy()
    spoils = {"null source": ("src", 0), "misaligned coefficients": ("coef", int(good[1]["coef"]) + 2), "zero width": ("width", 0),
              "size limit": ("height", J.MAX_SIDE + 1), "short stride": ("src_stride", 16), "two components": ("ncomp", 2), "sampling": ("hmax", 1),
              "another grid": ("bw", [2, 0, 0])}
    for what, (field, value) in spoils.items():
        table[:] = good
        table[1][field] = value
        with pytest.raises(RuntimeError, match="cft_jpeg_encode_coef"):
            J.jpeg_encode_coef(host.to(dev), host, 2)
        assert _lib.load().cft_last_error().decode().startswith("cft_jpeg_encode_coef"), what
    # a zero in the host copy of the tables
    tabs = keep[0].numpy().view(np.uint16).reshape(-1, 3, 64)
    saved = int(tabs[0, 0, 7])
    table[:] = good
    tabs[0, 0, 7] = 0
    with pytest.raises(RuntimeError, match="table entry"):
        J.jpeg_encode_coef(host.to(dev), host, 2)
    tabs[0, 0, 7] = saved
    torch.cuda.synchronize()
    assert (coef == 0x5A5A).all()                                     # the good first row was not encoded either
    J.jpeg_encode_coef(host.to(dev), host, 2)
    torch.cuda.synchronize()
    assert not (coef[:-64] == 0x5A5A).all() and (coef[-64:] == 0x5A5A).all()


# ---------------------------------------------------------------------------------------------------------------- detect(opt)
@pytest.fixture(scope="module")
def jpg_pairs(tmp_path_factory):
    """Four fixture pairs re-encoded as .jpg, a fifth kept as .png."""
    from PIL import Image
    root = tmp_path_factory.mktemp("jpg_pairs")
    names = sorted(os.listdir(os.path.join(DATA, "rgb", "images")))[:5]
    for stream in ("rgb", "ir"):
        os.makedirs(root / stream)
        for k, name in enumerate(names):
            src = os.path.join(DATA, stream, "images", name)
            if k == 4:
                shutil.copy(src, root / stream / name)
            else:
                with Image.open(src) as im:
                    im.convert("RGB").save(root / stream / (name[:-4] + ".jpg"), quality=90)
    return root


def _detect(jpg_pairs, project, name, device_jpeg, record=None):
    from msod_amd.detect import detect, make_parser
    opt = make_parser().parse_args(["--weights", CKPT, "--source1", str(jpg_pairs / "rgb"), "--source2", str(jpg_pairs / "ir"), "--img-size", "128",
                                    "--conf-thres", "0.001", "--save-txt", "--save-conf", "--project", str(project), "--name", name, "--batch-size", "2"])
    if device_jpeg is not None:
        opt.device_jpeg = device_jpeg
    lines = []
    save_dir = Path(detect(opt, log=lines.append, record=record))
    tidy = [re.sub(r"Done\. \(.*|Average Speed.*", "", ln).replace(str(save_dir), "<dir>") for ln in lines]
    return save_dir, tidy


def test_detect_with_device_jpeg_writes_pil_s_bytes(dev, jpg_pairs, tmp_path):
    from msod_amd.utils import jpeg as J
    want_dir, want_lines = _detect(jpg_pairs, tmp_path, "pil", None)                # the option absent: the default
    calls = []
    inner = J.jpeg_encode_coef

    def counted(table_dev, table_host, n):
        calls.append(n)
        return inner(table_dev, table_host, n)
    J.jpeg_encode_coef = counted
    try:
        got_dir, got_lines = _detect(jpg_pairs, tmp_path, "dev", True)
        rec = []
        rec_dir, _ = _detect(jpg_pairs, tmp_path, "rec", True, record=rec)
    finally:
        J.jpeg_encode_coef = inner
    assert sum(calls) == 8 + 8 and len(calls) < sum(calls)            # both streams of the four .jpg pairs, in batches; the .png pair is PIL's
    assert got_lines == want_lines
    files = sorted(f.name for f in want_dir.iterdir() if f.is_file())
    assert len(files) == 10 and sum(f.endswith(".jpg") for f in files) == 8 and sum(f.endswith(".png") for f in files) == 2
    for d in (got_dir, rec_dir):
        assert sorted(f.name for f in d.iterdir() if f.is_file()) == files
        for f in files:
            assert (d / f).read_bytes() == (want_dir / f).read_bytes(), f
        labels = sorted(f.name for f in (want_dir / "labels").iterdir())
        assert labels and sorted(f.name for f in (d / "labels").iterdir()) == labels
        for f in labels:
            assert (d / "labels" / f).read_text() == (want_dir / "labels" / f).read_text(), f
    assert len(rec) == 5 and all(r["drawn"] is not None for r in rec)  # record still receives the drawn originals


# ---------------------------------------------------------------------------------------------------------------- evaluate(plots=True)
def test_evaluate_plots_with_device_jpeg(dev, tmp_path):
    from msod_amd.evaluate import evaluate
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils import datasets as D
    from msod_amd.utils import plots as P
    from msod_amd.utils.seeded import seeded_state_dict
    model = Model(named_config("cfg2"))
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    model = model.to(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        loader, _ = D.create_dataloader_rgb_ir(os.path.join(DATA, "rgb", "images"), os.path.join(DATA, "ir", "images"), 64, 2, 32,
                                               SimpleNamespace(single_cls=True), pad=0.5, rect=True)
    batches = [(img.clone(), t.clone(), p, s) for img, t, p, s in loader]
    want = evaluate(model, batches, 1, single_cls=True, plots=True, save_dir=str(tmp_path / "pil"), names=["object"])
    got = evaluate(model, batches, 1, single_cls=True, plots=True, save_dir=str(tmp_path / "dev"), names=["object"], device_jpeg=True)
    np.testing.assert_equal(got[0], want[0])
    np.testing.assert_equal(np.asarray(got[1]), np.asarray(want[1]))
    files = sorted(f.name for f in (tmp_path / "pil").iterdir())
    assert files == sorted(f"test_batch{i}_{k}{s}.jpg" for i in range(3) for k in ("labels", "pred") for s in ("", "_ir"))
    assert sorted(f.name for f in (tmp_path / "dev").iterdir()) == files
    for f in files:
        assert (tmp_path / "dev" / f).read_bytes() == (tmp_path / "pil" / f).read_bytes(), f
    # plot_images by hand: the same switch, and a .png name stays on PIL
    img, targets, paths, _ = batches[0]
    P.plot_images(img.to(dev), targets, paths, str(tmp_path / "hand.jpg"), ["object"], device_jpeg=True)
    for s in ("", "_ir"):
        assert (tmp_path / f"hand{s}.jpg").read_bytes() == (tmp_path / "pil" / f"test_batch0_labels{s}.jpg").read_bytes()
    P.plot_images(img.to(dev), targets, paths, str(tmp_path / "a.png"), ["object"], device_jpeg=True)
    P.plot_images(img.to(dev), targets, paths, str(tmp_path / "b.png"), ["object"])
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
