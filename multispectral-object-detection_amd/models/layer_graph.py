"""The layer graph of a two-stream ``Model`` and every plan the executor derives from it.

The reference wires its layers through the yaml ``from`` field ``m.f``: ``-1`` = the previous layer's output, another negative int =
relative, a non-negative int = absolute, a list of those = several inputs, ``-4`` = the IR image ``x2`` (models/yolo_test.py:235-272;
row 0 consumes the RGB image ``x``).  ``LayerGraph`` is the only code that reads ``m.f``; ``Model.layer_graph()`` caches one per layer
list, so a structural edit (``nms()``, a sliced ``model.model``) rebuilds every plan at once.
"""
from functools import cached_property

import torch.nn as nn

from .common import GPT, SPP, Add, Add2, C3, Concat, Conv, Focus


def graph_key(layers):
    """Identity of a layer list (a ``LayerGraph`` holds its layers, so the ids of a live graph are not reused)."""
    return tuple(id(m) for m in layers)


class LayerGraph:
    def __init__(self, layers):
        self.layers = layers = list(layers)
        self.key = graph_key(layers)
        self.image = []          # 0: the layer consumes the RGB image x (row 0); 1: the IR image x2 (f == -4); None: layer outputs
        self.multi = []          # the layer takes a list of inputs
        self.sources = []        # absolute indices of the producers, in the order of ``f``
        for i, m in enumerate(layers):
            f = m.f
            self.image.append(1 if f == -4 else 0 if i == 0 else None)
            self.multi.append(not isinstance(f, int))
            self.sources.append([] if self.image[i] is not None else [i + j if j < 0 else j for j in ([f] if isinstance(f, int) else f)])
        self._segments = {}

    def inputs(self, i, prev, y):
        """Input of layer ``i``: ``prev`` (the output of layer i - 1, which ``y`` holds only if it is saved) and saved outputs ``y``."""
        vals = [prev if j == i - 1 else y[j] for j in self.sources[i]]
        return vals if self.multi[i] else vals[0]

    @cached_property
    def readers(self):
        """{producer index: set of the layers that read its output}."""
        readers = {}
        for j, srcs in enumerate(self.sources):
            for s in srcs:
                readers.setdefault(s, set()).add(j)
        return readers

    @cached_property
    def lanes(self):
        """Lane (HIP stream) of every layer: the IR backbone - everything reachable from an ``f == -4``
        entry through single-input edges, plus ``Add2(index=1)`` whose base input is the IR feature - is
        lane 1; joins (GPT, Add, Concat, Detect) and the RGB backbone/head are lane 0."""
        lanes = []
        for i, m in enumerate(self.layers):
            if self.image[i] is not None:
                lane = self.image[i]
            elif not self.multi[i] or isinstance(m, Add2):
                lane = lanes[self.sources[i][0]]
            else:
                lane = 0
            lanes.append(lane)
        return lanes

    def _cout(self, i, memo):
        """Output channels of layer ``i``, or None where it is never a planned concat source (GPT tuples, Detect, Sequentials)."""
        if i not in memo:
            m, srcs = self.layers[i], self.sources[i]
            if isinstance(m, Focus):
                c = m.conv.conv.out_channels
            elif type(m) is Conv:
                c = m.conv.out_channels
            elif isinstance(m, C3):
                c = m.cv3.conv.out_channels
            elif isinstance(m, SPP):
                c = m.cv2.conv.out_channels
            elif isinstance(m, Concat):
                c = sum(self._cout(j, memo) for j in srcs)
            elif isinstance(m, (Add, Add2)) or (isinstance(m, nn.Upsample) and not self.multi[i]):
                c = self._cout(srcs[0], memo)
            else:
                c = None
            memo[i] = c
        return memo[i]

    @cached_property
    def concat_plan(self):
        """{producer layer index: (concat layer index, channel offset, channels, total channels)} for every Concat
        source that is a Conv / C3 / Add (they take ``out=``); such a producer's output tensor then IS a channel
        slice of the concat buffer and ``Concat`` skips its copy.  Upsample sources stay deferred copies."""
        layers, plan, memo = self.layers, {}, {}
        try:
            for i, m in enumerate(layers):
                if not isinstance(m, Concat) or not self.multi[i]:
                    continue
                srcs = self.sources[i]
                chans = [self._cout(j, memo) for j in srcs]
                if any(c is None for c in chans):
                    continue
                off = 0
                for j, c in zip(srcs, chans):
                    if (type(layers[j]) is Conv or isinstance(layers[j], (C3, Add))) and j not in plan and self.image[j] != 1:
                        plan[j] = (i, off, c, sum(chans))
                    off += c
        except (IndexError, KeyError, TypeError, AttributeError):   # foreign module graph (bad `from` index, unknown
            plan = {}                                               # module type): no plan, Concat copies as before
        return plan

    @cached_property
    def chain_plan(self):
        """Indices of the ``Conv`` layers whose output is read by exactly one layer, the ``C3`` right behind them (``f == -1``).  Readers
        are counted from the ``f`` fields, not from ``Model.save``: the reference's ``x % i`` book-keeping (models/yolo_test.py:349) files
        the IR Focus's ``f = -4`` as a reader of row 1, which nothing reads."""
        layers = self.layers
        return frozenset(i for i, m in enumerate(layers[:-1])
                         if type(m) is Conv and type(layers[i + 1]) is C3 and layers[i + 1].f == -1 and self.readers.get(i) == {i + 1})

    @cached_property
    def cft_fusion_plan(self):
        """{index of the first Add2 behind a GPT block: (GPT index, index of the second Add2, index of the Add that consumes both
        or None)}.  The pattern is matched structurally; a config without it simply has no entries."""
        layers, sources, plan = self.layers, self.sources, {}
        pair = lambda j: self.multi[j] and len(sources[j]) == 2      # noqa: E731
        for i, m in enumerate(layers):
            if not isinstance(m, GPT) or not pair(i):
                continue
            adds = [j for j, a in enumerate(layers) if isinstance(a, Add2) and pair(j) and sources[j][1] == i]
            if len(adds) != 2 or {layers[adds[0]].index, layers[adds[1]].index} != {0, 1}:
                continue
            j1, j2 = adds
            if sources[j1][0] != sources[i][layers[j1].index] or sources[j2][0] != sources[i][layers[j2].index]:
                continue                               # an Add2 whose base is not the GPT's own input of that stream
            k = next((kk for kk, a in enumerate(layers) if type(a) is Add and self.multi[kk] and sorted(sources[kk]) == [j1, j2]), None)
            plan[j1] = (i, j2, k)
        return plan

    def prefix_segments(self, max_rows=None):
        """[(i0, i1)]: maximal runs of layers that depend on ONE image batch only - a ``Focus`` fed by ``x`` (row 0) or ``x2`` (``f == -4``)
        followed by ``f == -1`` Conv / C3 rows whose outputs have exactly one reader, the next row - cut to ``max_rows`` layers and
        to end on a C3 (a trailing Conv would be a ``PendingConv`` of a C3 outside the segment)."""
        segs = self._segments.get(max_rows)
        if segs is None:
            layers, readers, planned = self.layers, self.readers, self.concat_plan
            segs = self._segments[max_rows] = []
            for i0, m in enumerate(layers):
                if not isinstance(m, Focus) or self.image[i0] is None:
                    continue
                i1 = i0
                while (i1 + 1 < len(layers) and layers[i1 + 1].f == -1 and type(layers[i1 + 1]) in (Conv, C3) and readers.get(i1) == {i1 + 1}
                       and (i1 + 1) not in planned and (max_rows is None or i1 + 1 - i0 < max_rows)):
                    i1 += 1
                while i1 > i0 and type(layers[i1]) is not C3:
                    i1 -= 1
                if i1 > i0:
                    segs.append((i0, i1))
        return segs
