"""Guarded buffers for the memory-hygiene sweep (tests/test_gpu_memory_hygiene.py, self-tests in tests/test_guarded_host.py).

A kernel's result must depend only on its declared inputs and it must write only its declared outputs.  The value tests cannot see
either: they hand kernels fresh (mostly zero) memory, and a store past a tensor lands in somebody else's.  Here every device tensor
of a case lives inside one larger allocation, ``[band | payload | band]``; the bands, every output's prior content, every workspace
and the slack of a channel slice are filled with one byte, and the case runs once per byte of ``FILLS``:

    0x00  the baseline (what fresh memory usually looks like);
    0xFF  NaN in f32 / f16 / bf16, -1 in every integer type, 255 in u8: any arithmetic use of stray bytes shows;
    0x7B  a large positive finite value in all three float types (f16 0x7B7B = 61280, bf16 / f32 about 1.3e36) and a large positive
          int32: a stray value that a max, a softmax maximum, a score comparison or an atomicMax key lets win (a NaN is dropped
          there, as fmaxf drops it).

After each run: every status CFT_OK, every band intact (input bands included), every input unchanged bit for bit; across the runs the
defined part of every output bit-identical.  Every atomic in the kernels works on integers, so exact equality is justified.

Test code only: nothing here imports the oracle or the package.
"""
import torch

FILLS = (0x00, 0xFF, 0x7B)
MIN_BAND = 64 * 1024
BAND_ALIGN = 512


def _round_up(n, m):
    return -(-n // m) * m


class Guarded:
    """One allocation ``[band | payload | band]`` and the tensor ``t`` inside it.

    layout "dense": ``t`` is a contiguous tensor of ``shape``.  layout "nhwc": ``shape`` is the logical (B, C, H, W); the memory is
    NHWC with ``ld`` >= C channels per pixel and ``t`` is channels [off, off + C) of it - the other channels of every pixel count as
    band.  layout "rows": ``shape`` is (rows, C), row stride ``ld`` >= C, columns [off, off + C).  Each band is a multiple of 512
    bytes and at least max(64 KiB, payload bytes), so the overrun of a whole tile of rows still lands in memory this test owns, and the
    payload keeps the alignment of a fresh allocation."""

    def __init__(self, shape, dtype, dev, fill_byte, layout="dense", ld=None, off=0):
        shape = tuple(int(s) for s in shape)
        es = torch.empty((), dtype=dtype).element_size()
        if layout == "dense":
            full = shape
        elif layout == "nhwc":
            B, C, H, W = shape
            ld = C if ld is None else ld
            full = (B, H, W, ld)
        elif layout == "rows":
            R, C = shape
            ld = C if ld is None else ld
            full = (R, ld)
        else:
            raise ValueError(f"unknown layout {layout!r}")
        if layout != "dense" and not (0 <= off and off + C <= ld):
            raise ValueError(f"slice [{off}, {off + C}) does not fit {ld} channels")
        n = 1
        for s in full:
            n *= s
        self.payload_bytes = n * es
        self.band = _round_up(max(MIN_BAND, self.payload_bytes), BAND_ALIGN)
        self.fill = int(fill_byte)
        self.raw = torch.empty(2 * self.band + self.payload_bytes, dtype=torch.uint8, device=dev)
        self.raw.fill_(self.fill)
        pay = self.raw[self.band:self.band + self.payload_bytes].view(dtype).view(full)
        owned = torch.zeros(2 * self.band + self.payload_bytes, dtype=torch.bool, device=dev)
        own = owned[self.band:self.band + self.payload_bytes].view(full + (es,)) if n else None
        if layout == "dense":
            self.t = pay
            if n:
                own[...] = True
        elif layout == "nhwc":
            self.t = pay[..., off:off + C].permute(0, 3, 1, 2)
            if n:
                own[:, :, :, off:off + C] = True
        else:
            self.t = pay[:, off:off + C]
            if n:
                own[:, off:off + C] = True
        self._owned = owned
        self.ld, self.off = ld, off

    def bands_intact(self):
        """(ok, first differing byte offset within the allocation or None): every byte outside ``t``, compared on the device."""
        bad = (self.raw != self.fill) & ~self._owned
        if not bool(bad.any()):
            return True, None
        return False, int(bad.nonzero()[0])

    def where(self, offset):
        """Where a byte offset of the allocation lies relative to the payload, for the report."""
        if offset < self.band:
            return f"{self.band - offset} bytes before the payload"
        if offset >= self.band + self.payload_bytes:
            return f"{offset - self.band - self.payload_bytes} bytes past the payload"
        return f"payload byte {offset - self.band} (slack of the channel slice)"


def guarded(shape, dtype, dev, fill_byte, layout="dense", ld=None, off=0):
    return Guarded(shape, dtype, dev, fill_byte, layout, ld, off)


def _bytes(t):
    """The tensor's elements as a flat CPU byte tensor (bit comparison: NaNs compare by pattern)."""
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8)


class Run:
    """One run of a case under one fill byte: the case declares its device tensors here and launches on them."""

    def __init__(self, dev, fill):
        self.dev, self.fill = dev, fill
        self.items = []          # (kind, name, Guarded, cpu copy or None, defined)
        self.statuses = []
        self.held = []

    def _add(self, kind, name, g, cpu, defined=None):
        if any(n == name for _, n, *_ in self.items):
            raise ValueError(f"tensor {name!r} declared twice")
        self.items.append((kind, name, g, cpu, defined))
        return g.t

    def _filled(self, cpu, layout, ld, off):
        g = Guarded(cpu.shape, cpu.dtype, self.dev, self.fill, layout, ld, off)
        g.t.copy_(cpu)
        return g

    def inp(self, name, cpu, layout="dense", ld=None, off=0):
        """An input: the CPU tensor's values on the device; it must come back unchanged."""
        cpu = cpu.detach().clone()
        return self._add("in", name, self._filled(cpu, layout, ld, off), cpu)

    def inout(self, name, cpu, layout="dense", ld=None, off=0, defined=None):
        """An operand the kernel reads and writes: restored from its CPU copy before every run, compared across runs afterwards."""
        cpu = cpu.detach().clone()
        return self._add("inout", name, self._filled(cpu, layout, ld, off), cpu, defined)

    def out(self, name, shape, dtype, layout="dense", ld=None, off=0, defined=None):
        """An output: its prior content is the fill byte.  ``defined``: a bool mask (or ``f(outputs) -> mask``) of the part the header
        specifies - only where include/cft_hip.h calls the rest unspecified."""
        return self._add("out", name, Guarded(shape, dtype, self.dev, self.fill, layout, ld, off), None, defined)

    def work(self, name, shape, dtype=torch.uint8):
        """Scratch memory: poisoned with the fill byte; its contents afterwards do not matter, its bands do."""
        return self._add("work", name, Guarded(shape, dtype, self.dev, self.fill), None)

    def hold(self, *objects):
        """Keep host-side objects (descriptor tables whose address an entry point was given) alive until the run has been checked."""
        self.held.extend(objects)

    def status(self, st, what=""):
        """Record the return code of an entry point (all must be CFT_OK) under the entry point's name."""
        self.statuses.append((int(st), what))
        return st

    def tensor(self, name):
        for _, n, g, *_ in self.items:
            if n == name:
                return g.t
        raise KeyError(name)


def run_case(case, dev, fills=FILLS, launched=None):
    """Run ``case(run)`` once per fill byte.  Returns (problems, outputs of the first run as CPU tensors): ``problems`` is a list of
    strings, empty when the case is clean.  ``launched``: a set that receives the names the runs recorded with ``status``."""
    problems, first, first_fill, result = [], None, None, {}
    for fill in fills:
        run = Run(dev, fill)
        case(run)
        if torch.device(dev).type == "cuda":
            torch.cuda.synchronize()
        tag = f"fill 0x{fill:02X}"
        for st, what in run.statuses:
            if launched is not None:
                launched.add(what)
            if st != 0:
                problems.append(f"{tag}: status {st} {what}")
        if not run.statuses:
            problems.append(f"{tag}: the case recorded no status")
        outs = {}
        for kind, name, g, cpu, defined in run.items:
            ok, at = g.bands_intact()
            if not ok:
                problems.append(f"{tag}: band of {kind} '{name}' overwritten, first at {g.where(at)}")
            if kind == "in" and not torch.equal(_bytes(g.t), _bytes(cpu)):
                problems.append(f"{tag}: input '{name}' changed")
            if kind in ("out", "inout"):
                outs[name] = g.t.detach().cpu().clone()
        masked = {}
        for kind, name, g, cpu, defined in run.items:
            if kind not in ("out", "inout"):
                continue
            b = _bytes(outs[name])
            if defined is not None:
                m = defined(outs) if callable(defined) else defined
                m = m.expand(outs[name].shape).contiguous().reshape(-1)
                es = outs[name].element_size()
                b = torch.where(m.repeat_interleave(es), b, torch.zeros_like(b))
            masked[name] = b
        if first is None:
            first, first_fill, result = masked, fill, outs
        else:
            for name, b in masked.items():
                if not torch.equal(b, first[name]):
                    es = outs[name].element_size()
                    diff = (b != first[name]).nonzero().reshape(-1)
                    problems.append(f"{tag}: output '{name}' differs from the 0x{first_fill:02X} run at {int((diff // es).unique().numel())} "
                                    f"elements, first at flat index {int(diff[0]) // es}")
    return problems, result


def check_case(case, dev, fills=FILLS, launched=None):
    """Assert the case is clean; returns the outputs of the 0x00 run for a comparison with the kernel's reference."""
    problems, result = run_case(case, dev, fills, launched)
    assert not problems, "\n".join(problems)
    return result
