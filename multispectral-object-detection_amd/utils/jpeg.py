"""Baseline JPEG decoding with the entropy half on the host and the pixel half on the device (csrc/jpeg.hip, defined in
include/cft_hip.h): ``jpeg_info`` / ``jpeg_entropy`` wrap the two host functions - plain C++, callable without a GPU and from many
threads at once - and ``decode_jpeg_batch`` decodes a list of files with one upload and one ``cft_jpeg_decode_u8`` call (two launches).
A file outside the supported subset is reported as such, never decoded approximately: the caller hands it to PIL."""
import ctypes

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


def fill_desc(row, info, coef_ptr, qtab_ptr, dst_ptr, dst_stride, plane_off):
    """One JPEG_DESC row from a file's info and where its pieces live on the device."""
    row["coef"], row["qtab"], row["dst"], row["dst_stride"], row["plane_off"] = coef_ptr, qtab_ptr, dst_ptr, dst_stride, plane_off
    for k in ("width", "height", "ncomp", "hmax", "vmax", "bw", "bh"):
        row[k] = info[k]


def jpeg_decode_u8(table_dev, table_host, n, workspace):
    """Launch ``cft_jpeg_decode_u8`` on the current stream: ``table_dev`` / ``table_host`` uint8 tensors holding the same ``n`` JPEG_DESC
    rows on the device and on the host, ``workspace`` a uint8 CUDA tensor for the component planes."""
    if not table_dev.is_cuda or not workspace.is_cuda or table_host.is_cuda:
        raise RuntimeError("jpeg_decode_u8: table_dev and workspace live on the device, table_host on the host (this package runs on MI355X only)")
    for t in (table_dev, table_host):
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < n * JPEG_DESC.itemsize:
            raise ValueError(f"jpeg_decode_u8: a table is a contiguous uint8 tensor of at least {n} x {JPEG_DESC.itemsize} bytes")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise ValueError("jpeg_decode_u8: workspace must be a contiguous uint8 tensor")
    st = _lib.load().cft_jpeg_decode_u8(table_dev.data_ptr(), table_host.data_ptr(), n, workspace.data_ptr(), workspace.numel(),
                                        torch.cuda.current_stream(workspace.device).cuda_stream)
    _lib.check(st, "cft_jpeg_decode_u8")


def decode_jpeg_batch(blobs, device, out=None):
    """Decode the files ``blobs`` (bytes-like objects) on ``device``: a list with one HWC RGB uint8 CUDA tensor per file, or None in the
    slots whose file is outside the supported subset.  ``out``: optional list of destination tensors (None = allocate), each
    [h, w, 3] uint8 on the device with contiguous pixels; its row stride may be padded, the padding is not written.
    One pinned staging buffer, one non-blocking upload and one ``cft_jpeg_decode_u8`` call on the current stream; nothing here waits for
    the device, the returned tensors are ordered after the decode on that stream."""
    device = torch.device(device)
    infos = [jpeg_info(b) for b in blobs]
    offs, total = [], 0
    for info in infos:
        if info is None:
            offs.append(None)
            continue
        offs.append(total)
        total += _align16(2 * int(info["ncoef"])) + QTAB_BYTES
    results = [None] * len(blobs)
    if total == 0:
        return results
    pinned = torch.empty(total, dtype=torch.uint8).pin_memory()
    host = pinned.numpy()
    live = []
    for k, (blob, info, off) in enumerate(zip(blobs, infos, offs)):
        if info is None:
            continue
        nc = 2 * int(info["ncoef"])
        qoff = off + _align16(nc)
        if jpeg_entropy(blob, info, host[off:off + nc].view(np.int16), host[qoff:qoff + QTAB_BYTES].view(np.uint16)):
            live.append(k)
    if not live:
        return results
    table = np.zeros(len(live), dtype=JPEG_DESC)
    plane_total = sum(_align16(int(infos[k]["plane_bytes"])) for k in live)
    with torch.cuda.device(device):
        staged = pinned.to(device, non_blocking=True)
        workspace = torch.empty(plane_total, dtype=torch.uint8, device=device)
        plane_off = 0
        for row, k in zip(table, live):
            info = infos[k]
            h, w = int(info["height"]), int(info["width"])
            dst = out[k] if out is not None and out[k] is not None else torch.empty((h, w, 3), dtype=torch.uint8, device=device)
            if dst.dtype != torch.uint8 or tuple(dst.shape) != (h, w, 3) or dst.stride(2) != 1 or dst.stride(1) != 3 or dst.device != staged.device:
                raise ValueError(f"decode_jpeg_batch: out[{k}] must be a uint8 [{h}, {w}, 3] tensor on {device} with contiguous pixels")
            base = staged.data_ptr() + offs[k]
            fill_desc(row, info, base, base + _align16(2 * int(info["ncoef"])), dst.data_ptr(), dst.stride(0) if h > 1 else max(dst.stride(0), 3 * w), plane_off)
            plane_off += _align16(int(info["plane_bytes"]))
            results[k] = dst
        table_host = torch.from_numpy(table.view(np.uint8).reshape(-1)).pin_memory()
        table_dev = table_host.to(device, non_blocking=True)
        jpeg_decode_u8(table_dev, table_host, len(live), workspace)
    return results
