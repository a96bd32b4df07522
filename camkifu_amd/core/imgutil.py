"""Small array helpers of the host side (reference core/imgutil.py).  Here: CyclicBuffer (:533-656), the short history
SfMeta's regions keep of their states, scores and results."""
import numpy as np


class CyclicBuffer:
    """`size` arrays of one shape, kept as the slots of ONE array `buffer` whose last axis is the slot number.  Indexing
    the object reads and writes the CURRENT slot (`index % size`) -- the slot axis is implied and may not be named --
    while `buffer` shows all slots at once.  `increment` moves on to the next slot; its old content stays until it is
    overwritten."""

    def __init__(self, shape, size, dtype=None, init=None):
        dims = (shape,) if isinstance(shape, int) else tuple(shape)
        self.size, self.index = size, 0
        self.buffer = np.full(dims + (size,), 0 if init is None else init, dtype=dtype)

    def _slot(self, item):
        key = item if isinstance(item, tuple) else (item,)
        if len(key) >= self.buffer.ndim:
            raise AssertionError("the last axis is the slot of the cycle: it is implied, do not index it")
        pad = (slice(None),) * (self.buffer.ndim - 1 - len(key))
        return key + pad + (self.index % self.size,)

    def __getitem__(self, key):
        return self.buffer[self._slot(key)]

    def __setitem__(self, key, content):
        self.buffer[self._slot(key)] = content

    def replace(self, old, put):
        """the first slot AFTER the current one (cyclically, the current one last) whose content equals `old` gets `put`"""
        wanted = old if isinstance(old, np.ndarray) else np.array([old])
        for step in range(1, self.size + 1):
            k = (self.index + step) % self.size
            if np.array_equal(self.buffer[..., k], wanted):
                self.buffer[..., k] = put
                return

    def increment(self):
        self.index = self.index + 1

    def _slot_number(self):
        return self.index % self.size

    def at_start(self):
        return self._slot_number() == 0

    def at_end(self):
        return self._slot_number() == self.size - 1
