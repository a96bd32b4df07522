"""Small array helpers of the host side (reference core/imgutil.py).  Here: CyclicBuffer (:533-656), the short history
SfMeta's regions keep of their states, scores and results; and the two drawing helpers draw_lines (:71-92) and draw_str
(:95-118), which build a display list and hand it to the GPU rasteriser in one call (core/overlay.py)."""
import numpy as np

from .. import cvconf
from . import overlay


def _factor(img):
    """how many times the image would be pyrDown-ed to fit the screen (reference :162-175)"""
    f, width, height = 0, img.shape[1], img.shape[0]
    while cvconf.screenw < width or cvconf.screenh < height:
        f, width, height = f + 1, width / 2, height / 2
    return f


def lines_list(img, segments, color=255, into=None):
    """draw_lines' display list: every segment 1 + 2 * _factor(img) thick (reference :82)"""
    dl = into if into is not None else overlay.DisplayList()
    thickness = 1 + 2 * _factor(img)
    for seg in segments:
        if len(seg) == 4:
            (x0, y0), (x1, y1) = seg[0:2], seg[2:4]
        elif len(seg) == 2:
            (x0, y0), (x1, y1) = seg
        else:
            raise ValueError("Unrecognized segment format: {}".format(seg))
        dl.segment(x0, y0, x1, y1, color, thickness=thickness)
    return dl


def draw_lines(img, segments, color=255):
    """draw each segment -- 4 integers (x0, y0, x1, y1) or two couples ((x0, y0), (x1, y1)) -- on the image, in place.
    The path is the rasteriser's Bresenham rule, not cv2.line's clipped one ("Overlays")."""
    overlay.draw(img, lines_list(img, segments, color))


def str_list(dst, s, x=None, y=None, color=(255, 255, 255), into=None, scale=1):
    """draw_str's display list: a black copy at (x + 1, y + 1), then the coloured one.  (x, y) is the reference's origin,
    the text's baseline: the first cell's top is y - 7 * scale.  The defaults centre the string as the reference does
    (:110-114)."""
    dl = into if into is not None else overlay.DisplayList()
    if x is None:
        x = int(dst.shape[1] / 2 - len(s) * 3.5)
    if y is None:
        y = int(dst.shape[0] / 2 - 3)
    top = int(y) - 7 * scale
    dl.text(int(x) + 1, top + 1, s, (0, 0, 0), scale=scale)
    return dl.text(int(x), top, s, color, scale=scale)


def draw_str(dst, s, x=None, y=None, color=(255, 255, 255)):
    """print a string with a black shadow on the image, in place, in the project's 5 x 7 font at scale 1 (cv2.putText's
    antialiased Hershey strokes are not reproduced)"""
    overlay.draw(dst, str_list(dst, s, x, y, color))


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
