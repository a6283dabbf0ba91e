"""Baseline JPEG decoding with the entropy half on the host and the pixel half on the device (csrc/jpeg.hip, defined in
include/cft_hip.h): ``jpeg_info`` / ``jpeg_entropy`` wrap the two host functions - plain C++, callable without a GPU and from many
threads at once - and ``decode_jpeg_batch`` decodes a list of files with one upload and one ``cft_jpeg_decode_u8`` call (two launches).
A file outside the supported subset is reported as such, never decoded approximately: the caller hands it to PIL.

Encoding is the same seam in the other direction (csrc/jpeg_encode.hip): ``encode_jpeg_batch`` turns device images into the bytes
PIL's ``save(f, 'JPEG', quality=q, subsampling=s)`` writes - one table upload, one ``cft_jpeg_encode_coef`` launch, one non-blocking copy
of the coefficients into pinned memory, then ``cft_jpeg_write`` (headers and Huffman coding) on a pool of host threads;
``encode_jpeg_start`` / ``EncodeJob`` is the form that lets a caller overlap the copy and the coding with other work."""
import ctypes
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib

OK, UNSUPPORTED, EINVAL = _lib._consts["CFT_OK"], _lib._consts["CFT_JPEG_UNSUPPORTED"], _lib._consts["CFT_EINVAL"]
QTAB_BYTES = _lib._consts["CFT_JPEG_QTAB_BYTES"]
MAX_SIDE = _lib._consts["CFT_JPEG_MAX_SIDE"]
# cft_jpeg_info_t of include/cft_hip.h
JPEG_INFO = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"),
                      ("restart_interval", "<i4"), ("hs", "<i4", (3,)), ("vs", "<i4", (3,)), ("bw", "<i4", (3,)), ("bh", "<i4", (3,)),
                      ("cw", "<i4", (3,)), ("ch", "<i4", (3,)), ("reserved", "<i4", (2,)), ("ncoef", "<i8"), ("plane_bytes", "<i8")])
# one row of the table cft_jpeg_decode_u8 reads: cft_jpeg_desc_t of include/cft_hip.h
JPEG_DESC = np.dtype([("coef", "<u8"), ("qtab", "<u8"), ("dst", "<u8"), ("dst_stride", "<i8"), ("plane_off", "<i8"), ("width", "<i4"), ("height", "<i4"),
                      ("ncomp", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"), ("bw", "<i4", (3,)), ("bh", "<i4", (3,)), ("reserved", "<i4", (3,))])
assert JPEG_INFO.itemsize == _lib._consts["CFT_JPEG_INFO_BYTES"] and JPEG_DESC.itemsize == _lib._consts["CFT_JPEG_DESC_BYTES"]
# one row of the table cft_jpeg_encode_coef reads: cft_jpeg_enc_desc_t of include/cft_hip.h
JPEG_ENC_DESC = np.dtype([("src", "<u8"), ("qtab", "<u8"), ("qtab_host", "<u8"), ("coef", "<u8"), ("src_stride", "<i8"), ("width", "<i4"), ("height", "<i4"),
                          ("ncomp", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"), ("bw", "<i4", (3,)), ("bh", "<i4", (3,)), ("reserved", "<i4", (3,))])
assert JPEG_ENC_DESC.itemsize == _lib._consts["CFT_JPEG_ENC_DESC_BYTES"]
SHORT_BUFFER = _lib._consts["CFT_JPEG_SHORT_BUFFER"]
SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}      # luma (hmax, vmax); the integers are PIL's
MAX_ENCODE_THREADS = 16
JPEG_SUFFIXES = (".jpg", ".jpeg")


def _align16(n):
    return (n + 15) & ~15


def _as_bytes(blob):
    """A uint8 numpy view of bytes / bytearray / memoryview / uint8 array (no copy for contiguous input)."""
    a = blob if isinstance(blob, np.ndarray) else np.frombuffer(blob, dtype=np.uint8)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError("JPEG bytes must be a bytes-like object or a one-dimensional uint8 array")
    return np.ascontiguousarray(a)


def jpeg_info(blob):
    """``cft_jpeg_info`` on the bytes of one file: a one-element JPEG_INFO record (``info["width"]``, ...), or None when the file is not
    in the supported subset (progressive, CMYK, not a JPEG, ...: the caller decodes it with PIL).  Needs no GPU."""
    a = _as_bytes(blob)
    info = np.zeros((), dtype=JPEG_INFO)
    st = _lib.load().cft_jpeg_info(a.ctypes.data, a.size, info.ctypes.data)
    if st == UNSUPPORTED:
        return None
    if st != OK:
        raise ValueError(f"cft_jpeg_info: status {st} (empty input)")
    return info


def jpeg_entropy(blob, info, coef, qtab):
    """``cft_jpeg_entropy``: Huffman-decode the file into ``coef`` (int16, ``info["ncoef"]`` values) and ``qtab`` (uint16, 192 values),
    both writable contiguous numpy arrays (views of pinned memory in the loader).  True on success, False when the entropy data puts
    the file outside the subset (truncated, corrupt, a coefficient beyond 16 bits after dequantisation).  Needs no GPU."""
    a = _as_bytes(blob)
    if coef.dtype != np.int16 or coef.size != int(info["ncoef"]) or not coef.flags.c_contiguous or not coef.flags.writeable:
        raise ValueError(f"jpeg_entropy: coef must be a writable contiguous int16 array of {int(info['ncoef'])} values")
    if qtab.dtype != np.uint16 or qtab.size != QTAB_BYTES // 2 or not qtab.flags.c_contiguous or not qtab.flags.writeable:
        raise ValueError(f"jpeg_entropy: qtab must be a writable contiguous uint16 array of {QTAB_BYTES // 2} values")
    st = _lib.load().cft_jpeg_entropy(a.ctypes.data, a.size, coef.ctypes.data, qtab.ctypes.data, info.ctypes.data)
    if st == UNSUPPORTED:
        return False
    if st != OK:
        raise ValueError(f"cft_jpeg_entropy: status {st} (info does not belong to these bytes)")
    return True


def fill_geometry(row, info):
    """The geometry fields both tables share (JPEG_DESC, JPEG_ENC_DESC), copied from a file's info into one row."""
    for k in ("width", "height", "ncomp", "hmax", "vmax", "bw", "bh"):
        row[k] = info[k]


def fill_desc(row, info, coef_ptr, qtab_ptr, dst_ptr, dst_stride, plane_off):
    """One JPEG_DESC row from a file's info and where its pieces live on the device."""
    row["coef"], row["qtab"], row["dst"], row["dst_stride"], row["plane_off"] = coef_ptr, qtab_ptr, dst_ptr, dst_stride, plane_off
    fill_geometry(row, info)


def _check_tables(who, table_dev, table_host, n, itemsize):
    if not table_dev.is_cuda or table_host.is_cuda:
        raise RuntimeError(f"{who}: table_dev lives on the device, table_host on the host (this package runs on MI355X only)")
    for t in (table_dev, table_host):
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < n * itemsize:
            raise ValueError(f"{who}: a table is a contiguous uint8 tensor of at least {n} x {itemsize} bytes")


def jpeg_decode_u8(table_dev, table_host, n, workspace):
    """Launch ``cft_jpeg_decode_u8`` on the current stream: ``table_dev`` / ``table_host`` uint8 tensors holding the same ``n`` JPEG_DESC
    rows on the device and on the host, ``workspace`` a uint8 CUDA tensor for the component planes."""
    _check_tables("jpeg_decode_u8", table_dev, table_host, n, JPEG_DESC.itemsize)
    if not workspace.is_cuda:
        raise RuntimeError("jpeg_decode_u8: workspace lives on the device (this package runs on MI355X only)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("jpeg_decode_u8: workspace must be a contiguous uint8 tensor")
    st = _lib.load().cft_jpeg_decode_u8(table_dev.data_ptr(), table_host.data_ptr(), n, workspace.data_ptr(), workspace.numel(),
                                        torch.cuda.current_stream(workspace.device).cuda_stream)
    _lib.check(st, "cft_jpeg_decode_u8")


# Where the files of one decode call sit: coef_off / qtab_off per file in the pinned upload (None for a file PIL decodes), upload_bytes
# its size, plane_bytes per file in the plane workspace (0 for PIL's) and their sum plane_total.
DecodePlan = namedtuple("DecodePlan", "coef_off qtab_off upload_bytes plane_bytes plane_total")


def decode_plan(infos, reserve=0):
    """The staging plan of ``infos`` (``jpeg_info`` records, None for a file PIL has to decode): ``reserve`` bytes for the caller's table
    rows, then per file the coefficients and the quantisation tables, every offset and plane size a multiple of 16 (the C guards)."""
    coef_off, qtab_off, plane_bytes, total = [], [], [], _align16(reserve)
    for info in infos:
        if info is None:
            coef_off.append(None), qtab_off.append(None), plane_bytes.append(0)
            continue
        coef_off.append(total)
        qtab_off.append(total + _align16(2 * int(info["ncoef"])))
        total = qtab_off[-1] + QTAB_BYTES
        plane_bytes.append(_align16(int(info["plane_bytes"])))
    return DecodePlan(coef_off, qtab_off, total, plane_bytes, sum(plane_bytes))


def entropy_staged(blob, info, host, plan, k):
    """``jpeg_entropy`` of file ``k`` of the plan into its place in ``host``, the uint8 numpy view of the pinned upload."""
    c0, q0 = plan.coef_off[k], plan.qtab_off[k]
    return jpeg_entropy(blob, info, host[c0:c0 + 2 * int(info["ncoef"])].view(np.int16), host[q0:q0 + QTAB_BYTES].view(np.uint16))


def fill_decode_rows(table, plan, infos, live, upload_ptr, dsts):
    """The JPEG_DESC rows of the files ``live`` (indices into the plan), the upload at the device address ``upload_ptr``, ``dsts`` the
    ``(pointer, row stride)`` of each destination.  Their planes follow one another from 0; returns where the last one ends."""
    plane_off = 0
    for row, k, (dst_ptr, dst_stride) in zip(table, live, dsts):
        fill_desc(row, infos[k], upload_ptr + plan.coef_off[k], upload_ptr + plan.qtab_off[k], dst_ptr, dst_stride, plane_off)
        plane_off += plan.plane_bytes[k]
    return plane_off


def decode_jpeg_batch(blobs, device, out=None):
    """Decode the files ``blobs`` (bytes-like objects) on ``device``: a list with one HWC RGB uint8 CUDA tensor per file, or None in the
    slots whose file is outside the supported subset.  ``out``: optional list of destination tensors (None = allocate), each
    [h, w, 3] uint8 on the device with contiguous pixels; its row stride may be padded, the padding is not written.
    One pinned staging buffer, one non-blocking upload and one ``cft_jpeg_decode_u8`` call on the current stream; nothing here waits for
    the device, the returned tensors are ordered after the decode on that stream."""
    device = torch.device(device)
    infos = [jpeg_info(b) for b in blobs]
    plan = decode_plan(infos)
    results = [None] * len(blobs)
    if plan.upload_bytes == 0:
        return results
    pinned = torch.empty(plan.upload_bytes, dtype=torch.uint8).pin_memory()
    host = pinned.numpy()
    live = [k for k, info in enumerate(infos) if info is not None and entropy_staged(blobs[k], info, host, plan, k)]
    if not live:
        return results
    table = np.zeros(len(live), dtype=JPEG_DESC)
    with torch.cuda.device(device):
        staged = pinned.to(device, non_blocking=True)
        dsts = []
        for k in live:
            h, w = int(infos[k]["height"]), int(infos[k]["width"])
            dst = out[k] if out is not None and out[k] is not None else torch.empty((h, w, 3), dtype=torch.uint8, device=device)
            if dst.dtype != torch.uint8 or tuple(dst.shape) != (h, w, 3) or dst.stride(2) != 1 or dst.stride(1) != 3 or dst.device != staged.device:
                raise ValueError(f"decode_jpeg_batch: out[{k}] must be a uint8 [{h}, {w}, 3] tensor on {device} with contiguous pixels")
            dsts.append((dst.data_ptr(), dst.stride(0) if h > 1 else max(dst.stride(0), 3 * w)))
            results[k] = dst
        workspace = torch.empty(fill_decode_rows(table, plan, infos, live, staged.data_ptr(), dsts), dtype=torch.uint8, device=device)
        table_host = torch.from_numpy(table.view(np.uint8).reshape(-1)).pin_memory()
        table_dev = table_host.to(device, non_blocking=True)
        jpeg_decode_u8(table_dev, table_host, len(live), workspace)
    return results


# ---------------------------------------------------------------------------------------------------------------- encoding
def jpeg_layout(width, height, ncomp, hmax=1, vmax=1):
    """``cft_jpeg_layout``: the JPEG_INFO record of a file to be written.  Needs no GPU."""
    info = np.zeros((), dtype=JPEG_INFO)
    if _lib.load().cft_jpeg_layout(int(width), int(height), int(ncomp), int(hmax), int(vmax), info.ctypes.data) != OK:
        raise ValueError(f"jpeg_layout: {width} x {height}, {ncomp} component(s) sampled {hmax}x{vmax} is outside what the encoder writes "
                         f"(sides 1..{MAX_SIDE}; grey 1x1, colour 1x1 / 2x1 / 2x2)")
    return info


def jpeg_quality_tables(quality):
    """``cft_jpeg_quality_tables``: uint16 [3, 64], natural order, rows luminance / chrominance / chrominance.  Needs no GPU."""
    qtab = np.zeros((3, 64), dtype=np.uint16)
    if _lib.load().cft_jpeg_quality_tables(int(quality), qtab.ctypes.data) != OK:
        raise ValueError(f"jpeg_quality_tables: quality {quality} outside 1..100")
    return qtab


def jpeg_write_bound(info):
    """``cft_jpeg_write_bound``: a byte count no file laid out as ``info`` exceeds.  Needs no GPU."""
    bound = ctypes.c_long(0)
    if _lib.load().cft_jpeg_write_bound(info.ctypes.data, ctypes.byref(bound)) != OK:
        raise ValueError("jpeg_write_bound: info was not made by jpeg_layout")
    return bound.value


def jpeg_write(coef, qtab, info):
    """``cft_jpeg_write``: the bytes of the file whose quantised coefficients are ``coef`` (contiguous int16, ``info["ncoef"]`` values, the
    layout of ``jpeg_entropy``).  Needs no GPU; callable from many threads at once (the call releases the GIL)."""
    lib = _lib.load()
    if coef.dtype != np.int16 or coef.size != int(info["ncoef"]) or not coef.flags.c_contiguous:
        raise ValueError(f"jpeg_write: coef must be a contiguous int16 array of {int(info['ncoef'])} values")
    if qtab.dtype != np.uint16 or qtab.size != QTAB_BYTES // 2 or not qtab.flags.c_contiguous:
        raise ValueError(f"jpeg_write: qtab must be a contiguous uint16 array of {QTAB_BYTES // 2} values")
    cap = jpeg_write_bound(info)
    out = np.empty(cap, dtype=np.uint8)
    n = ctypes.c_long(0)
    st = lib.cft_jpeg_write(coef.ctypes.data, qtab.ctypes.data, info.ctypes.data, out.ctypes.data, cap, ctypes.byref(n))
    if st != OK:
        raise ValueError(f"jpeg_write: status {st} ({'a coefficient outside the baseline range' if st == UNSUPPORTED else 'bad tables or info'})")
    return out[:n.value].tobytes()


def jpeg_encode_coef(table_dev, table_host, n):
    """Launch ``cft_jpeg_encode_coef`` on the current stream: ``table_dev`` / ``table_host`` uint8 tensors holding the same ``n``
    JPEG_ENC_DESC rows on the device and on the host."""
    _check_tables("jpeg_encode_coef", table_dev, table_host, n, JPEG_ENC_DESC.itemsize)
    st = _lib.load().cft_jpeg_encode_coef(table_dev.data_ptr(), table_host.data_ptr(), n, torch.cuda.current_stream(table_dev.device).cuda_stream)
    _lib.check(st, "cft_jpeg_encode_coef")


class EncodeJob:
    """What ``encode_jpeg_start`` leaves behind: the coefficients of every image on their way into pinned memory.  ``file_bytes(k)``
    waits for the copy (an event, not the device) and codes image ``k`` on the calling thread - any thread, several at once."""

    def __init__(self, infos, offsets, qtab, pinned, event, keep):
        self.infos, self.offsets, self.qtab, self.pinned, self.event = infos, offsets, qtab, pinned, event
        self._keep = keep                                  # the sources and device buffers stay alive until the copy is done
        self._host = pinned.numpy()

    def __len__(self):
        return len(self.infos)

    def wait(self):
        self.event.synchronize()
        self._keep = None

    def coefficients(self, k):
        """The int16 coefficients of image ``k`` (a view of the pinned buffer) once the copy has arrived."""
        self.event.synchronize()
        return self._host[self.offsets[k]:self.offsets[k] + int(self.infos[k]["ncoef"])]

    def file_bytes(self, k):
        return jpeg_write(self.coefficients(k), self.qtab, self.infos[k])

    def save(self, k, path):
        """Code image ``k`` and write the file ``path``."""
        data = self.file_bytes(k)
        with open(path, 'wb') as f:
            f.write(data)

    def all_bytes(self, pool=None):
        if pool is not None:
            out = list(pool.map(self.file_bytes, range(len(self))))
        elif len(self) == 1:
            out = [self.file_bytes(0)]
        else:
            with ThreadPoolExecutor(min(MAX_ENCODE_THREADS, len(self))) as own:
                out = list(own.map(self.file_bytes, range(len(self))))
        self._keep = None
        return out


def encode_jpeg_start(images, quality=75, subsampling="4:2:0"):
    """The device stage of ``encode_jpeg_batch``: ``images`` are uint8 CUDA tensors of one device, [h, w, 3] RGB or grey ([h, w] or
    [h, w, 1]), of mixed sizes; a view whose rows are strided (padded rows, a crop) is read in place, anything else is made contiguous.
    One pinned buffer with the tables and the descriptor rows, one upload, one ``cft_jpeg_encode_coef`` launch and one non-blocking copy
    of all coefficients into pinned memory on the current stream, then an event.  Nothing here waits for the device.  Returns an
    ``EncodeJob``."""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"encode_jpeg: subsampling {subsampling!r} is not one of '4:4:4', '4:2:2', '4:2:0' (or PIL's 0, 1, 2)")
    if not len(images):
        raise ValueError("encode_jpeg: no images")
    qtab = jpeg_quality_tables(quality)
    device = images[0].device
    srcs, infos, offsets, total = [], [], [], 0
    for k, im in enumerate(images):
        if not torch.is_tensor(im) or not im.is_cuda or im.dtype != torch.uint8 or im.device != device or im.dim() not in (2, 3) or \
                (im.dim() == 3 and im.shape[2] not in (1, 3)):
            raise ValueError(f"encode_jpeg: images[{k}] must be a uint8 CUDA tensor [h, w, 3], [h, w, 1] or [h, w] on {device}")
        if im.dim() == 2:
            im = im.unsqueeze(2)
        h, w, nc = im.shape
        if im.stride(2) != 1 or im.stride(1) != nc or (h > 1 and im.stride(0) < nc * w):
            im = im.contiguous()
        hmax, vmax = SUBSAMPLING[subsampling] if nc == 3 else (1, 1)
        info = jpeg_layout(w, h, nc, hmax, vmax)
        srcs.append(im)
        infos.append(info)
        offsets.append(total)
        total += int(info["ncoef"])                        # a multiple of 64 values: every image starts on a 128-byte boundary
    n = len(srcs)
    head = QTAB_BYTES + n * JPEG_ENC_DESC.itemsize
    staging = torch.empty(head, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    host[:QTAB_BYTES].view(np.uint16)[:] = qtab.reshape(-1)
    table = host[QTAB_BYTES:].view(JPEG_ENC_DESC)
    with torch.cuda.device(device):
        staged = torch.empty(head, dtype=torch.uint8, device=device)
        coef = torch.empty(total, dtype=torch.int16, device=device)
        for row, im, info, off in zip(table, srcs, infos, offsets):
            h, w, nc = im.shape
            row["src"], row["qtab"], row["qtab_host"], row["coef"] = im.data_ptr(), staged.data_ptr(), staging.data_ptr(), coef.data_ptr() + 2 * off
            row["src_stride"] = im.stride(0) if h > 1 else max(im.stride(0), nc * w)
            fill_geometry(row, info)
            row["reserved"] = 0
        staged.copy_(staging, non_blocking=True)
        jpeg_encode_coef(staged[QTAB_BYTES:], staging[QTAB_BYTES:], n)
        pinned = torch.empty(total, dtype=torch.int16).pin_memory()
        pinned.copy_(coef, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
    return EncodeJob(infos, offsets, qtab, pinned, event, (srcs, staged, staging, coef))


def encode_jpeg_batch(images, quality=75, subsampling="4:2:0", pool=None):
    """The bytes of ``Image.fromarray(a).save(f, 'JPEG', quality=quality, subsampling=subsampling)`` for every image of ``images``
    (``encode_jpeg_start``), byte for byte: a list of ``bytes``.  ``pool``: an executor for the host coding (default: up to 16 threads
    of its own).  ``Image.save`` without options is quality 75 at 4:2:0."""
    return encode_jpeg_start(images, quality, subsampling).all_bytes(pool)


def is_jpeg_name(path):
    return str(path).lower().endswith(JPEG_SUFFIXES)
