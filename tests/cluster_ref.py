"""Plain restatement of SfClustering.find_stones (reference stone/sf_clustering.py:48-168) and of the library call under it,
cv2.kmeans(pixels, 3, None, (TERM_CRITERIA_EPS, 15, 3), 3, KMEANS_PP_CENTERS) as OpenCV 3.1.0 runs it: the generator, the
k-means++ seeding, the passes with the empty-cluster rule, the masked ratios, interpret_ratios and check_density.  numpy,
with the library's SEQUENTIAL sums (np.cumsum adds in order), sharing no code with the product.  Test-only.

Also `ClusterRefCtx`: a stand-in for capi.Context on a CPU-only host that answers `cluster_stones` from this file and
everything else from the oracle (tests/stub_ctx.py)."""
import numpy as np

GS = 19
F32 = np.float32
MASK64 = (1 << 64) - 1


class RNG:
    """cv::RNG: a 64-bit multiply-with-carry; the default seed is 0xffffffff"""

    def __init__(self, state=0xffffffff):
        self.state = int(state) & MASK64

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + (self.state >> 32)) & MASK64
        return self.state & 0xffffffff

    def real(self):
        return self.next() * 2.0 ** -32

    def advanced(self, draws):
        r = RNG(self.state)
        for _ in range(draws):
            r.next()
        return r.state


def sqdist(a, b):
    """normL2Sqr of 3-vectors in f32: ((0 + v0^2) + v1^2) + v2^2; a (N, 3) f32, b (3,) f32 -> (N,) f32"""
    v = a - b[None, :]
    s = v[:, 0] * v[:, 0]
    s = s + v[:, 1] * v[:, 1]
    s = s + v[:, 2] * v[:, 2]
    return s


def seq_sum(x, dtype):
    """the last of the running sums: additions in index order, each rounded to dtype"""
    x = np.asarray(x, dtype)
    if len(x) == 0:
        return np.zeros(x.shape[1:], dtype)
    return np.cumsum(x, axis=0, dtype=dtype)[-1]


def seed_pp(px, rng):
    """generateCentersPP: indices of the 3 seeded centres (7 draws)"""
    n = len(px)
    first = rng.next() % n
    centers = [first]
    dist = sqdist(px, px[first])
    sum0 = float(seq_sum(dist, np.float64))
    for _ in range(2):
        best_sum, best_c, best_d = np.inf, -1, None
        for _trial in range(3):
            p = rng.real() * sum0
            # for (i = 0; i < N - 1; i++) if ((p -= dist[i]) <= 0) break;
            run = np.cumsum(np.concatenate([[p], -dist[:n - 1].astype(np.float64)]))[1:]
            hit = np.nonzero(run <= 0)[0]
            ci = int(hit[0]) if len(hit) else n - 1
            td = np.minimum(sqdist(px, px[ci]), dist)
            s = float(seq_sum(td, np.float64))
            if s < best_sum:
                best_sum, best_c, best_d = s, ci, td
        centers.append(best_c)
        dist, sum0 = best_d, best_sum
    return centers


def kmeans3(px, rng, int_sums=False, max_passes=100, eps2=9.0, farthest_last=True, first_min=True):
    """px: (N, 3) f32.  -> dict(labels (N,) uint8, centers (3, 3) f32, passes [3], compactness [3], winner)
    int_sums: the per-cluster channel sums are the exact sums rounded once to f32 (what the GPU gives above 65 793 pixels
    of uint8 input, where a sequential f32 sum is no longer exact) instead of the library's sequential f32 sums.
    farthest_last / first_min: the two tie rules, switchable so that the tests can show they matter."""
    px = np.ascontiguousarray(px, F32)
    n = len(px)
    best = dict(compactness=np.inf)
    passes, comps = [], []
    for attempt in range(3):
        centers = px[seed_pp(px, rng)].copy()
        labels = np.zeros(n, np.int32)
        shift, it, comp = np.inf, 0, 0.0
        while True:
            if it > 0:
                old = centers
                counts = np.bincount(labels, minlength=3).astype(np.int64)
                if int_sums:
                    sums = np.stack([px[labels == k].astype(np.float64).sum(0) for k in range(3)]).astype(F32)
                else:
                    sums = np.stack([seq_sum(px[labels == k], F32) for k in range(3)])
                for k in range(3):
                    if counts[k] != 0:
                        continue
                    mk = 0
                    for k1 in range(1, 3):
                        if counts[mk] < counts[k1]:
                            mk = k1
                    oc = sums[mk] * (F32(1.0) / F32(counts[mk]))
                    idx = np.nonzero(labels == mk)[0]
                    d = sqdist(px[idx], oc)
                    far = idx[np.nonzero(d == d.max())[0][-1 if farthest_last else 0]]
                    counts[mk] -= 1
                    counts[k] += 1
                    labels[far] = k
                    sums[mk] = sums[mk] - px[far]
                    sums[k] = sums[k] + px[far]
                centers = np.stack([sums[k] * (F32(1.0) / F32(counts[k])) for k in range(3)]).astype(F32)
                shift = 0.0
                for k in range(3):
                    t = centers[k] - old[k]
                    tt = t * t
                    d = 0.0
                    for c in range(3):
                        d += float(tt[c])
                    shift = max(shift, d)
            it += 1
            if it == max(max_passes, 2) or shift <= eps2:
                break
            d = np.stack([sqdist(px, centers[k]) for k in range(3)], 1)
            if first_min:
                labels = np.argmin(d, 1).astype(np.int32)
            else:
                labels = (2 - np.argmin(d[:, ::-1], 1)).astype(np.int32)
            comp = float(seq_sum(d[np.arange(n), labels], np.float64))
        passes.append(it)
        comps.append(comp)
        if comp < best["compactness"]:
            best = dict(compactness=comp, labels=labels.astype(np.uint8), centers=centers.copy(), winner=attempt)
    return dict(labels=best["labels"], centers=best["centers"], winner=best["winner"], passes=passes, compactness=comps)


def circle_mask(rects, side):
    """StonesFinder.getmask (stonesfinder.py:452-490): a disc in every zone, zones written in raster order; pixels no zone
    covers are 0"""
    mask = np.zeros((side, side), np.uint8)
    for r in range(GS):
        for c in range(GS):
            x0, y0, x1, y1 = (int(v) for v in rects[r][c])
            h, w = mask[x0:x1, y0:y1].shape
            a, b = h / 2, w / 2
            rad = min(a, b)
            y, x = np.ogrid[-a:h - a, -b:w - b]
            mask[x0:x1, y0:y1] = x * x + y * y <= rad * rad
    return mask


def grey_levels(centers):
    return [int(((F32(c[0]) + F32(c[1])) + F32(c[2])) / F32(3)) for c in np.asarray(centers, F32)]


def find_stones(img, rects, mask, rs=0, re=GS, cs=0, ce=GS, rng=None, int_sums=False, rounding=False, **rules):
    """-> dict(stones (19, 19) uint8 0 E / 1 B / 2 W, trusted, ratios (19, 19, 3) uint8, centers, labels (hs, ws) uint8,
    passes, compactness, winner).  Compactness 0 (the reference fails there): stones all E, not trusted."""
    rng = rng if rng is not None else RNG()
    rects = np.asarray(rects).reshape(GS, GS, 4)
    x0, y0 = int(rects[rs, cs, 0]), int(rects[rs, cs, 1])
    x1, y1 = int(rects[re - 1, ce - 1, 2]), int(rects[re - 1, ce - 1, 3])
    sub = np.asarray(img)[x0:x1, y0:y1].astype(F32)
    hs, ws = sub.shape[:2]
    km = kmeans3(sub.reshape(hs * ws, 3), rng, int_sums=int_sums, **rules)
    vals = grey_levels(km["centers"])
    labels = km["labels"].reshape(hs, ws).astype(np.int32) + 1
    labels = labels * mask[x0:x1, y0:y1].astype(np.int32)
    ratios = np.zeros((GS, GS, 3), np.uint8)
    ratios[:, :, vals.index(sorted(vals)[1])] = 1
    for x in range(rs, re):
        for y in range(cs, ce):
            a0, b0, a1, b1 = (int(v) for v in rects[x, y])
            zone = labels[a0 - x0:a1 - x0, b0 - y0:b1 - y0]
            for lab in range(1, 4):
                cnt = int(np.count_nonzero(zone == lab))
                if cnt:
                    q = 100 * cnt / zone.size
                    ratios[x, y, lab - 1] = int(round(q)) if rounding else int(q)
    colours = [1 if g == min(vals) else 2 if g == max(vals) else 0 for g in vals]
    stones = np.zeros((GS, GS), np.uint8)
    for i in range(rs, re):
        for j in range(cs, ce):
            stones[i, j] = colours[int(np.argmax(ratios[i, j]))]
    trusted = check_density(stones)
    if min(km["compactness"]) == 0:
        stones, trusted = np.zeros((GS, GS), np.uint8), False
    return dict(stones=stones, trusted=trusted, ratios=ratios, centers=km["centers"], labels=km["labels"].reshape(hs, ws),
                passes=km["passes"], compactness=km["compactness"], winner=km["winner"])


def check_density(stones):
    vals, counts = np.unique(stones, return_counts=True)
    return bool(len(vals) == 3 and counts.min() >= 2)


def attempts_separated(compactness, rel=1e-9):
    """the condition on a test input: any two attempts' compactness values are bit-equal or differ by more than `rel`
    relative, so that a fixed-order double sum and a sequential one rank the attempts alike"""
    c = list(compactness)
    for i in range(3):
        for k in range(i + 1, 3):
            if c[i] != c[k] and abs(c[i] - c[k]) <= rel * max(abs(c[i]), abs(c[k])):
                return False
    return True


def default_rects(side=380):
    """StonesFinder.getrect of the default grid (stonesfinder.py:412-450, 964-981), restated: intersections at cell
    centres, zones bounded halfway towards the diagonal neighbours"""
    half = side / GS / 2
    pos = [int((half * (GS - 1 - i) + (side - half) * i) / (GS - 1)) for i in range(GS)]
    out = np.zeros((GS, GS, 4), np.int32)
    for r in range(GS):
        for c in range(GS):
            p = (pos[r], pos[c])
            pb = (pos[r - 1] if r else -pos[0], pos[c - 1] if c else -pos[0])
            pa = (pos[r + 1] if r < GS - 1 else 2 * side - pos[r] - 2, pos[c + 1] if c < GS - 1 else 2 * side - pos[c] - 2)
            out[r, c] = (max(0, int((pb[0] + p[0]) / 2)), max(0, int((pb[1] + p[1]) / 2)),
                         min(side, int((p[0] + pa[0]) / 2)), min(side, int((p[1] + pa[1]) / 2)))
    return out


def _stub_base():
    from tests.stub_ctx import OracleCtx
    return OracleCtx


class ClusterRefCtx(_stub_base()):
    """OracleCtx + cluster_stones / rng_state answered by this file (same arguments and results as capi.Context)"""

    def __init__(self):
        super().__init__()
        self.rng_state = 0xffffffff
        self.cluster_calls = []

    def cluster_stones(self, goban, rects, mask, jobs=None, rs=0, re=GS, cs=0, ce=GS, want_all=False):
        goban = np.asarray(goban)
        single = goban.ndim == 3
        imgs = goban[None] if single else goban
        plain = jobs is None
        if plain:
            jobs = [(f, rs, re, cs, ce) for f in range(len(imgs))]
        jobs = np.asarray(jobs, np.int32).reshape(-1, 5)
        self.cluster_calls.append(jobs.copy())
        res = []
        for j, (f, a, b, c, d) in enumerate(jobs):
            res.append(find_stones(imgs[f], rects, mask, a, b, c, d, rng=RNG(RNG(self.rng_state).advanced(21 * j))))
        self.rng_state = RNG(self.rng_state).advanced(21 * len(jobs))
        stones = np.stack([r["stones"] for r in res])
        trusted = np.array([r["trusted"] for r in res], bool)
        extra = dict(ratios=np.stack([r["ratios"] for r in res]), centers=np.stack([r["centers"] for r in res]),
                     labels=[r["labels"] for r in res], passes=np.array([r["passes"] for r in res], np.int32),
                     compactness=np.array([r["compactness"] for r in res], np.float64),
                     winner=np.array([r["winner"] for r in res], np.int32))
        if single and plain:
            stones, trusted = stones[0], bool(trusted[0])
        return (stones, trusted, extra) if want_all else (stones, trusted)
