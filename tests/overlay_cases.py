"""Display lists built for the branches of the overlay rasteriser, as raw (P, 8) int32 rows (no library code): every case
is the list of ONE frame of h x w, scaled to the shape asked for; `seam` is where two bins meet (the bin size of the
plan).  cases(h, w, seam) -> [(name, prims, text)]; batch(h, w, seam) -> (prims, frame_start, text) of three frames."""
import numpy as np

SEGMENT, CIRCLE, DISC, RECT, TEXT = 1, 2, 3, 4, 5
FAR = 32767


def col(b, g, r, alpha=255):
    v = b | g << 8 | r << 16 | alpha << 24
    return v - (1 << 32) if v >= 1 << 31 else v


def seg(x0, y0, x1, y1, t=1, colour=col(255, 255, 255)):
    return (SEGMENT, x0, y0, x1, y1, t, colour, 0)


def circle(x, y, r, t=1, colour=col(0, 255, 255)):
    return (CIRCLE, x, y, t, 0, r, colour, 0)


def disc(x, y, r, colour=col(255, 0, 255)):
    return (DISC, x, y, 0, 0, r, colour, 0)


def rect(x0, y0, x1, y1, size=1, colour=col(0, 0, 255)):
    return (RECT, x0, y0, x1, y1, size, colour, 0)


class _Text:
    def __init__(self):
        self.bytes = bytearray()

    def __call__(self, x, y, raw, s=1, colour=col(255, 255, 255)):
        row = (TEXT, x, y, len(raw), 0, s, colour, len(self.bytes))
        self.bytes += raw
        return row


def cases(h, w, seam=32, seed=5):
    rng = np.random.RandomState(seed)
    cx, cy, m = w // 2, h // 2, min(h, w) - 1
    out = []

    def add(name, rows, text=b""):
        out.append((name, np.array(rows, np.int64).reshape(-1, 8).astype(np.int32), bytes(text)))

    add("axes", [seg(1, cy, w - 2, cy), seg(cx, h - 2, cx, 1, colour=col(10, 20, 30)), seg(w + 3, cy + 1, -4, cy + 1, 3)])
    add("diagonals", [seg(0, 0, m, m), seg(m, 0, 0, m, colour=col(9, 99, 199)), seg(cx + 5, cy + 5, cx - 5, cy - 5, 3)])
    star = []
    for k, (a, b) in enumerate([(7, 3), (3, 7)]):
        for j, (sa, sb) in enumerate([(1, 1), (1, -1), (-1, 1), (-1, -1)]):
            star.append(seg(cx, cy, cx + sa * a, cy + sb * b, colour=col(30 * (k * 4 + j) + 20, 255 - 25 * j, 40 + 50 * k)))
    add("star", star)
    # the exact half-way ties and their mirrors (x <-> y, left <-> right, up <-> down)
    ties = []
    for (a, b) in [(2, 1), (4, 2)]:
        for k, (ex, ey) in enumerate([(a, b), (-a, b), (a, -b), (-a, -b), (b, a), (-b, a), (b, -a), (-b, -a)]):
            ox, oy = 6 + 12 * (k % 4), 6 + 12 * (k // 4) + (0 if a == 2 else 1)
            ties.append(seg(ox, oy, ox + ex, oy + ey, colour=col(255, 40 * k, 17 * a)))
    add("ties", ties)
    add("ties_at_origin", [seg(0, 0, 2, 1), seg(0, 0, 4, 2, colour=col(1, 2, 3)), seg(2, 1, 0, 0, colour=col(50, 60, 70))])
    add("points", [seg(3, 3, 3, 3), seg(0, 0, 0, 0, 3, col(1, 200, 3)), seg(w - 1, h - 1, w - 1, h - 1, 7, col(200, 1, 3)),
                   seg(-2, -2, -2, -2, 7)])
    add("far_endpoints", [seg(-FAR, cy - 16000, FAR, cy + 16001), seg(cx - 9000, -FAR, cx + 9001, FAR, colour=col(0, 255, 0)),
                          seg(FAR, cy - 3, -FAR, cy + 4, 3, col(255, 0, 0)), seg(-FAR, -FAR, FAR, FAR, 7, col(5, 6, 7)),
                          seg(cx, -FAR, cx + 1, FAR, colour=col(77, 7, 177))])
    add("outside", [seg(-50, -50, -10, -5), seg(w + 5, 0, w + 40, h, 7), seg(-FAR, -FAR, -FAR, FAR), seg(0, h + 4, w, h + 4, 7)])
    thick = [seg(2, 2 + 9 * k, w - 3, 5 + 9 * k, t, col(255 - 60 * k, 80 * k, 128)) for k, t in enumerate((1, 3, 7))]
    thick += [seg(seam - 3, 1, seam + 3, h - 2, 7, col(12, 34, 56)), seg(1, seam + 1, w - 2, seam - 2, 3, col(65, 43, 21))]
    add("thick", thick)
    spots = [(0, 0), (w - 1, h - 1), (seam, seam), (seam - 1, cy), (-20, -20), (w + 3, cy), (cx, cy)]
    rings, discs = [], []
    for k, (x, y) in enumerate(spots):
        for j, r in enumerate((0, 1, 2, 5, 10)):
            rings.append(circle(x + 3 * j * (k == 6), y, r, 1, col(40 * j + 30, 250 - 30 * k, 30 * k)))
            discs.append(disc(x, y + 2 * j * (k == 6), r, col(30 * k, 40 * j + 30, 250 - 30 * k)))
    add("rings", rings)
    add("thick_rings", [circle(x, y, r, t) for (x, y) in spots[:4] for r, t in ((0, 3), (1, 3), (2, 5), (5, 3), (10, 7), (3, 15))])
    add("discs", discs[::-1])
    add("rects", [rect(w - 3, h - 2, 2, 1), rect(2, 2, 10, 8, 5, col(0, 255, 0)), rect(-5, -5, 3, 3, 0, col(255, 0, 0)),
                  rect(seam - 2, seam + 2, seam + 6, seam - 3, 2, col(9, 9, 9)), rect(cx, cy, cx, cy, 1), rect(w, h, w + 5, h + 5, 0),
                  rect(-FAR, cy, FAR, cy + 2, 1, col(200, 100, 0)), rect(1, h - 1, w - 2, h - 1, 3, col(3, 2, 1))])
    t = _Text()
    add("text", [t(-7, 2, b"Frame 12/345 ~{|} wide enough to run off the right edge of any test image"),
                 t(3, h - 9, b"gj,Q@ off the bottom", 2, col(0, 200, 255)), t(1, 11, bytes([31, 65, 127, 200, 66]), 1, col(255, 0, 0)),
                 t(seam - 4, seam - 3, b"#seam$", 2, col(0, 255, 0)), t(2, 2, b""), t(w + 1, 0, b"out"), t(0, -40, b"above", 3)], t.bytes)
    add("order", [rect(1, 1, w - 2, h - 2, 0, col(10, 20, 30)), disc(cx, cy, 6, col(255, 255, 255, 96)),
                  rect(cx - 2, cy - 9, cx + 2, cy + 9, 0, col(0, 0, 255)), disc(cx - 3, cy, 4, col(200, 0, 0, 128)),
                  disc(cx + 3, cy, 4, col(0, 200, 0, 127)), seg(0, cy, w - 1, cy, 3, col(255, 255, 0, 1)),
                  seg(0, 0, w - 1, h - 1, 1, col(0, 255, 255, 254))])
    n = 24
    add("seeded", [seg(*rng.randint(-8, max(w, h) + 8, 4), t=int(rng.choice([1, 3, 5])), colour=col(*rng.randint(0, 256, 3), int(rng.randint(1, 256))))
                   for _ in range(n)]
        + [circle(int(rng.randint(-4, w + 4)), int(rng.randint(-4, h + 4)), int(rng.randint(0, 14)), int(rng.choice([1, 3])),
                  col(*rng.randint(0, 256, 3), int(rng.randint(1, 256)))) for _ in range(n)])
    return out


def batch(h, w, seam=32):
    """three frames with three different lists, the middle one empty"""
    by_name = {name: (p, t) for name, p, t in cases(h, w, seam)}
    first, text = by_name["text"]
    last = by_name["order"][0]
    prims = np.concatenate([first, last])
    return prims, np.array([0, len(first), len(first), len(prims)], np.int32), text


def as_batch(prims):
    return np.array([0, len(prims)], np.int32)
