"""Display lists: what the finders' drawing helpers build and capi.Context.overlay_draw rasterises on the GPU.

A DisplayList is the ordered list of primitives of ONE image; pack() turns one list per frame into the three arrays of
ck_overlay_draw (include/camkifu_amd.h, "overlays"):
    prims        int32 (P, 8) = kind, x0, y0, x1, y1, size, colour, aux     colour = b | g << 8 | r << 16 | alpha << 24
    frame_start  int32 (n + 1,), CSR: frame f owns prims[frame_start[f]:frame_start[f + 1]]
    text         bytes: a TEXT primitive's aux is its offset there, x1 its length
Coordinates are integer pixels (x to the right, y down, as cv2 takes points) and may lie outside the image.  The rules
of every primitive -- the Bresenham path of a segment, the discs, the 6s x 8s text cells of the project's own 5 x 7
font -- and the two deviations from cv2 are in DESIGN.md, "Overlays".  Nothing here needs a GPU."""
import numpy as np

SEGMENT, CIRCLE, DISC, RECT, TEXT = 1, 2, 3, 4, 5          # CK_OV_*
CELL_W, CELL_H = 6, 8                                       # a text cell at scale 1; the glyph is the 5 x 7 in its top-left


def colour_code(color, alpha=255):
    """an int (grey: b = g = r) or a (b, g, r) sequence of numbers, truncated to integers and clamped to 0 .. 255, and an
    alpha of 1 .. 255 -> the packed colour"""
    if np.isscalar(color):
        color = (color, color, color)
    b, g, r = (min(255, max(0, int(v))) for v in tuple(color)[:3])
    return b | g << 8 | r << 16 | (int(alpha) & 255) << 24


class DisplayList:
    """the primitives of one image, in painting order.  Every method returns the list itself."""

    def __init__(self):
        self.prims = []             # rows of 8 ints; a TEXT row carries its bytes in place of aux until pack()

    def __len__(self):
        return len(self.prims)

    def _add(self, kind, x0, y0, x1, y1, size, color, alpha, aux=0):
        self.prims.append((kind, int(x0), int(y0), int(x1), int(y1), int(size), colour_code(color, alpha), aux))
        return self

    def segment(self, x0, y0, x1, y1, color=255, thickness=1, alpha=255):
        return self._add(SEGMENT, x0, y0, x1, y1, thickness, color, alpha)

    def circle(self, x, y, radius, color=255, thickness=1, alpha=255):
        return self._add(CIRCLE, x, y, thickness, 0, radius, color, alpha)

    def disc(self, x, y, radius, color=255, alpha=255):
        return self._add(DISC, x, y, 0, 0, radius, color, alpha)

    def rect(self, x0, y0, x1, y1, color=255, thickness=1, alpha=255):
        """corners inclusive, in either order; thickness 0 fills"""
        return self._add(RECT, x0, y0, x1, y1, thickness, color, alpha)

    def text(self, x, y, s, color=255, scale=1, alpha=255):
        """(x, y): the top-left corner of the first cell.  A str is written as latin-1 where it can be; whatever has no
        glyph (a byte outside 32 .. 126) is drawn as '?'."""
        raw = s if isinstance(s, (bytes, bytearray)) else str(s).encode("latin-1", "replace")
        return self._add(TEXT, x, y, len(raw), 0, scale, color, alpha, bytes(raw))

    def extend(self, other):
        self.prims.extend(other.prims)
        return self


def pack(lists):
    """one DisplayList per frame -> (prims (P, 8) int32, frame_start (n + 1,) int32, text bytes)"""
    rows, start, text = [], [0], bytearray()
    for dl in lists:
        for p in dl.prims:
            if p[0] == TEXT:
                rows.append(p[:7] + (len(text),))
                text += p[7]
            else:
                rows.append(p)
        start.append(len(rows))
    prims = np.array(rows, np.int64).reshape(-1, 8)
    prims[:, 6] = np.where(prims[:, 6] >= 1 << 31, prims[:, 6] - (1 << 32), prims[:, 6])     # the colour's bits as int32
    return prims.astype(np.int32), np.array(start, np.int32), bytes(text)


def unpack(prims, frame_start, text):
    """the inverse of pack -> a list of DisplayList"""
    out = []
    for f in range(len(frame_start) - 1):
        dl = DisplayList()
        for p in np.asarray(prims).reshape(-1, 8)[frame_start[f]:frame_start[f + 1]]:
            p = tuple(int(v) for v in p)
            colour = p[6] & 0xffffffff
            dl.prims.append(p[:6] + (colour, bytes(text[p[7]:p[7] + p[3]]) if p[0] == TEXT else p[7]))
        out.append(dl)
    return out


def draw(img, display_list, ctx=None):
    """one library call: `display_list` rasterised on `img` (numpy, or a torch tensor in HBM), in place, on `ctx` or the
    process-wide context -> img"""
    if not len(display_list):
        return img
    if ctx is None:
        from .. import capi
        ctx = capi.get_context()
    return ctx.overlay_draw(img, display_list)
