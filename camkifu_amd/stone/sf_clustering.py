"""SfClustering for the MI355X: the k-means stones finder under its registration name (reference
stone/sf_clustering.py:8-184).

`find_stones` -- 3-means over the BGR pixels of a board region (cv2.kmeans, k-means++ seeding, three attempts), the share of
each cluster under the circle mask of every intersection zone, darkest cluster black / brightest white / the other empty,
and the density check that says whether three clusters made sense at all -- is ONE library call for any number of regions
of any number of goban images (`ck_cluster_stones`, camkifu_amd/csrc/k_cluster.hip): the whole iterative loop of a region
runs inside one workgroup of one kernel launch.  The library reproduces the generator of the stones thread (cv::RNG, state
in the context), so results are those of the reference call for call.

Run on its own the finder averages frames and submits the whole board from columns 6-13 every third frame, as the
reference does; SfMeta uses `find_stones` / `find_stones_regions` directly."""
import numpy as np

from .. import capi
from ..golib_shim import gsize, E, B, W
from ..host import stones_finder_base

_SYMBOL = np.array([E, B, W], dtype=object)


class SfClustering(stones_finder_base()):

    def __init__(self, vmanager, ctx=None):
        try:
            super().__init__(vmanager, learn_bg=vmanager is not None, ctx=ctx)
        except TypeError:                                   # the host application's base takes no ctx
            super().__init__(vmanager)
            self.ctx = ctx if ctx is not None else capi.Context(getattr(vmanager, "device", 0))
        # accu: f32 running average of the goban frames; last: what the last library call answered (ratios, centers, ...)
        self.accu, self.last = None, None

    # ---- the frame loop of the finder run on its own -----------------------------------------------------------
    def _find(self, goban_img):
        frame = np.asarray(goban_img)
        fresh = frame.astype(np.float32)
        # cv2.accumulateWeighted(frame, accu, 0.2), in f32 like the library
        self.accu = fresh if self.accu is None else self.accu * np.float32(0.8) + fresh * np.float32(0.2)
        if self.total_f_processed % 3 == 0:
            stones = self.find_stones(self.accu, 0, gsize, 6, 13)
            if stones is None:
                return
            self.bulk_update([(stones[r][c], r, c) for r in range(gsize) for c in range(gsize)])

    def _learn(self):
        pass

    # ---- the library call -------------------------------------------------------------------------------------------
    def zone_table(self):
        grid = getattr(self, "_posgrid", None)
        if hasattr(grid, "zones"):
            return np.ascontiguousarray(grid.zones(1.0), np.int32)
        return np.array([[self.getrect(r, c) for c in range(gsize)] for r in range(gsize)], np.int32)

    def _prepared(self, img):
        """uint8 images go as they are, anything else as float32 (the reference converts everything to float32: for bytes
        the result is the same bit for bit)"""
        if capi._is_torch(img):
            return img
        img = np.asarray(img)
        return np.ascontiguousarray(img) if img.dtype == np.uint8 else np.ascontiguousarray(img, np.float32)

    def _call(self, img, jobs):
        stones, trusted, extra = self.ctx.cluster_stones(self._prepared(img), self.zone_table(), self.getmask(), jobs=jobs,
                                                         want_all=True)
        self.last = dict(extra, stones=stones, trusted=trusted)
        return stones, trusted, extra

    def find_stones(self, img, rs=0, re=gsize, cs=0, ce=gsize, **kwargs):
        """-> (19, 19) object array of B / W / E (E outside rows [rs, re) x columns [cs, ce)), or None when the result is
        not to be trusted (check_density).  Extra keyword arguments are accepted and ignored, as in the reference."""
        stones, trusted, _ = self._call(img, [(0, rs, re, cs, ce)])
        return _SYMBOL[stones[0]] if trusted[0] else None

    def find_stones_regions(self, img, regions):
        """several regions (rs, re, cs, ce) of one image in ONE call, in the order given (which is the order their random
        numbers are drawn in) -> list of find_stones answers"""
        if not len(regions):
            return []
        stones, trusted, _ = self._call(img, [(0,) + tuple(reg) for reg in regions])
        return [_SYMBOL[s] if t else None for s, t in zip(stones, trusted)]

    def find_stones_batch(self, imgs, rs=0, re=gsize, cs=0, ce=gsize, jobs=None):
        """n goban images (host arrays or device tensors), one region each -- or an explicit job list of (image, rs, re, cs,
        ce) rows -> stones uint8 (m, 19, 19) of 0 E / 1 B / 2 W, trusted bool (m,)"""
        if jobs is None:
            jobs = [(f, rs, re, cs, ce) for f in range(len(imgs))]
        return self.ctx.cluster_stones(self._prepared(imgs), self.zone_table(), self.getmask(), jobs=jobs)

    # ---- the reference's steps, answered by the library (API the host application may call) -------------------------
    def cluster_colors(self, img, rs=0, re=gsize, cs=0, ce=gsize):
        """-> ratios (19, 19, 3) uint8: per intersection the percentage of each cluster; centers (3, 3) float32: the BGR
        centre of each cluster, in the order of the ratios' last axis"""
        _, _, extra = self._call(img, [(0, rs, re, cs, ce)])
        return extra["ratios"][0], extra["centers"][0]

    def interpret_ratios(self, ratios, centers, r_start=0, r_end=gsize, c_start=0, c_end=gsize):
        """one colour per zone: the cluster with the largest share (the first of equals); clusters are named by the grey
        level of their centre -- darkest B, brightest W, the other E"""
        if len(centers) != 3:
            raise AssertionError("three clusters, three centres")
        grey = [int((np.float32(c[0]) + np.float32(c[1]) + np.float32(c[2])) / np.float32(3)) for c in centers]
        names = [B if g == min(grey) else W if g == max(grey) else E for g in grey]
        stones = np.full((gsize, gsize), E, dtype=object)
        best = np.argmax(np.asarray(ratios)[r_start:r_end, c_start:c_end], axis=2)
        stones[r_start:r_end, c_start:c_end] = np.array(names, dtype=object)[best]
        return stones

    def check_density(self, stones):
        """three colours on the board, each at least twice: otherwise 3-means had nothing to separate"""
        _, counts = np.unique(np.asarray(stones, dtype=object).astype(str), return_counts=True)
        return len(counts) == 3 and int(counts.min()) >= 2

    def _window_name(self):
        return SfClustering.__name__
