"""Launch tracer of the model executor's tests: the sequence of library calls and stream waits that a walk issues.

``with recording(device) as events:`` replaces ``_lib.load`` by a proxy of the loaded library and patches
``torch.cuda.Stream.wait_stream`` for the duration of the block.  Every ``cft_*`` call appends ``"<entry point> <lane> <digest>"``: the
lane is 0 for the stream that was current when the block began and 1 for any other, the digest covers the scalar arguments and, for
pointer arguments (``c_void_p`` in ``_lib.SIGNATURES``), only whether they are null.  Every ``wait_stream`` appends
``"wait_stream <waiting lane> <awaited lane>"`` in sequence with the launches - under HIP-graph capture these waits are the edges
between the two branches of the graph.  Names and lanes are in clear so that a mismatch names the first differing event."""
import ctypes
import hashlib
from contextlib import contextmanager

import torch


class _Proxy:
    def __init__(self, lib, signatures, record):
        self._lib, self._signatures, self._record, self._wrapped = lib, signatures, record, {}

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            fn = getattr(self._lib, name)
            if name in self._signatures:
                fn = self._wrap(name, fn, self._signatures[name][1])
            self._wrapped[name] = fn
        return fn

    def _wrap(self, name, fn, argtypes):
        is_ptr = [t is ctypes.c_void_p for t in argtypes]

        def call(*args):
            what = tuple(bool(a) if p else a for a, p in zip(args, is_ptr))
            self._record(f"{name} %d {hashlib.sha1(repr(what).encode()).hexdigest()[:8]}")
            return fn(*args)
        return call


@contextmanager
def recording(device):
    from msod_amd import _lib
    main = torch.cuda.current_stream(device)
    events = []

    def lane(stream=None):
        return 0 if (stream or torch.cuda.current_stream(device)) == main else 1

    real_load, real_wait = _lib.load, torch.cuda.Stream.wait_stream
    proxy = _Proxy(real_load(), _lib.SIGNATURES, lambda ev: events.append(ev % lane()))

    def wait_stream(self, other):
        events.append(f"wait_stream {lane(self)} {lane(other)}")
        return real_wait(self, other)

    _lib.load, torch.cuda.Stream.wait_stream = (lambda: proxy), wait_stream
    try:
        yield events
    finally:
        _lib.load, torch.cuda.Stream.wait_stream = real_load, real_wait


def first_difference(got, want):
    """None when the traces are equal, else a message that names the first differing event."""
    for n, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"event {n}: got '{g}', recorded '{w}' (after '{got[n - 1] if n else 'start'}')"
    if len(got) > len(want):
        return f"{len(got)} events, recorded {len(want)}; first extra: '{got[len(want)]}'"
    if len(got) < len(want):
        return f"{len(got)} events, recorded {len(want)}; first missing: '{want[len(got)]}'"
    return None
