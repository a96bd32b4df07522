"""SfMeta for the MI355X: the stones finder that combines contour analysis and k-means clustering, region by region, under
its registration name (reference stone/sf_meta.py:19-470).  It is the reference's only ACTING finder that needs no trained
model.

The goban is cut into 3 x 3 regions (rows / columns 0-6, 6-12, 12-19).  Each region carries a short cyclic history
(length 3) of states -- warmup, search, idle -- of what each delegate found, and of how k-means fared there:
    * too much foreground on the region or around it: nothing is looked for, and the region will search again later;
    * warmup: contour analysis, three calm frames; then search: the region's current finder, three calm frames; then idle
      until the foreground moves;
    * once the goban holds four stones in the region, k-means is TRIED beside the current finder (checked for thickness,
      against the known stones and against the grid lines); when a cycle of three tries scores >= 0 in sum the region
      switches to k-means;
    * a stone is submitted when it shows in enough of the last three results of a finder (`Region.commit`).

This is control flow over 19 x 19 arrays and stays Python, like stone/checks.py.  The pixel work is the two delegates':
SfContours (one library call per region that needs it) and SfClustering.  Which regions need k-means in a frame follows from
their state, the stones known at the start of the frame and the foreground alone, and no region needs it twice: so `_find`
first PLANS the nine regions, issues ONE `ck_cluster_stones` call for all of them -- in region order, which is the order
the reference would have drawn their random numbers in -- and then lets the regions act in raster order."""
import math

import numpy as np

from .. import capi
from ..core.exceptions import CorrectionWarning, DeletedError
from ..core.imgutil import CyclicBuffer
from ..golib_shim import gsize, E
from ..host import stones_finder_base
from .sf_clustering import SfClustering
from .sf_contours import SfContours

Warmup, Search, Idle = "warmup", "search", "idle"
_UNSET = object()


class SfMeta(stones_finder_base()):

    def __init__(self, vmanager, ctx=None):
        try:
            super().__init__(vmanager, ctx=ctx)
        except TypeError:                                   # the host application's base takes no ctx
            super().__init__(vmanager)
            self.ctx = ctx if ctx is not None else capi.Context(getattr(vmanager, "device", 0))
        # the delegates work on this finder's context and see this finder's foreground
        self.cluster = SfClustering(None, ctx=self.ctx)
        self.contour = SfContours(vmanager, ctx=self.ctx)
        for hook in ("get_foreground", "_show"):
            setattr(self.contour, hook, getattr(self, hook))
        self.routine_constr = {self.cluster: (self.check_against, self.check_flow), self.contour: (self.check_flow,)}
        self.split, self.histo = 3, 3
        self.regions = np.empty((self.split, self.split), dtype=object)
        for row, col in np.ndindex(self.regions.shape):
            self.regions[row, col] = Region(self, self.subregion(row, col), self.histo, finder=self.contour, state=Warmup)

    def _find(self, goban_img):
        if self.bg_init_frames > self.total_f_processed:    # the background model is still being sampled
            return
        known = self.get_stones()
        regions = list(self.regions.flat)
        wanted = [reg for reg in regions if reg.plan(known)]
        answers = self.cluster_regions(goban_img, [reg.bounds for reg in wanted])
        clustered = {id(reg): ans for reg, ans in zip(wanted, answers)}
        for reg in regions:
            reg.act(goban_img, known, clustered.get(id(reg), _UNSET))

    def cluster_regions(self, img, bounds):
        """k-means stones of several regions of one image, in order: one library call where the delegate offers it"""
        if not bounds:
            return []
        together = getattr(self.cluster, "find_stones_regions", None)
        if together is not None:
            return together(img, bounds)
        return [self.cluster.find_stones(img, rs=a, re=b, cs=c, ce=d) for a, b, c, d in bounds]

    def _learn(self):
        try:
            return super()._learn()
        except CorrectionWarning as unhandled:              # nothing here can learn from it yet
            print(str(unhandled))

    def subregion(self, row, col):
        """-> rs, re, cs, ce (ends exclusive) of region (row, col): `split` equal steps, the last one taking the rest"""
        if not (0 <= row < self.split and 0 <= col < self.split):
            raise AssertionError("region (%d, %d) of a %d x %d split" % (row, col, self.split, self.split))
        step = gsize // self.split

        def span(k):
            end = (k + 1) * step
            return k * step, gsize if gsize - end < step else end
        return span(row) + span(col)

    def _window_name(self):
        return SfMeta.__name__


class Region:
    """One rectangle of intersections [rs, re) x [cs, ce) and everything SfMeta remembers about it: `finder` (the delegate
    in charge), `states` / `contour_accu` / `cluster_accu` / `cluster_score` (cyclic histories of length `histo`),
    `population` (stones on the goban when k-means was last tried)."""

    def __init__(self, sf, boundaries, histo, finder=None, state=None):
        self.sf, self.histo, self.finder = sf, histo, finder
        self.bounds = tuple(int(v) for v in boundaries)
        self.rs, self.re, self.cs, self.ce = self.bounds
        cells = (self.re - self.rs, self.ce - self.cs)
        self.states = CyclicBuffer(1, histo, dtype=object, init=state)
        self.contour_accu = CyclicBuffer(cells, histo, dtype=object, init=E)
        self.cluster_accu = CyclicBuffer(cells, histo, dtype=object, init=E)
        self.accus = {sf.contour: self.contour_accu, sf.cluster: self.cluster_accu}
        self.cluster_score = CyclicBuffer(1, histo, dtype=np.int8)
        self.population, self.calm, self.trying = -1, True, False

    def _kwargs(self, canvas=None):
        return dict(rs=self.rs, re=self.re, cs=self.cs, ce=self.ce, canvas=canvas)

    def _inside(self, stones):
        return stones[self.rs:self.re, self.cs:self.ce]

    # ---- a frame, in two halves ------------------------------------------------------------------------------------
    def plan(self, ref_stones):
        """look at the foreground (which may reset the states) and say whether this frame needs k-means here"""
        self.calm, self.trying = self.check_foreground(), False
        if not self.calm or self.states[0] != Search:
            return False
        self.trying = self.clustering_needs_try(ref_stones)
        return self.trying or self.finder is self.sf.cluster

    def act(self, img, ref_stones, clustered=_UNSET, canvas=None):
        """search as the current state says, with the k-means answer `plan` asked for, and move on in the cycle; an
        agitated frame changes nothing and does not advance the cycle"""
        if not self.calm:
            return
        state = self.states[0]
        if state == Warmup:                                 # a few rounds of contour analysis to begin with
            history = self.contour_accu
            history[:] = self._inside(self.sf.contour.find_stones(img, **self._kwargs(canvas)))
            self.commit(history)
        elif state == Search:
            if self.trying:
                self.try_clustering(img, ref_stones, clustered)
            if not self.trying or self.finder is not self.sf.cluster:
                self.routine(img, ref_stones, clustered=clustered, canvas=canvas)
        follows = {Warmup: Search, Search: Idle}.get(state)
        if follows is not None:
            self.states[0] = follows                        # what this slot asks for when the cycle comes round again
        self.states.increment()

    def process(self, img, ref_stones, canvas=None):
        """the reference's entry point: both halves for this region alone"""
        clustered = _UNSET
        if self.plan(ref_stones):
            clustered = self.sf.cluster_regions(img, [self.bounds])[0]
        self.act(img, ref_stones, clustered, canvas)

    def _clustered(self, img, answer):
        return self.sf.cluster_regions(img, [self.bounds])[0] if answer is _UNSET else answer

    def routine(self, img, refs, clustered=_UNSET, canvas=None):
        """the current finder's result, cleaned of lonely first-line stones, checked, recorded and committed"""
        if self.finder is self.sf.cluster:
            stones = self._clustered(img, clustered)
        else:
            stones = self.finder.find_stones(img, **self._kwargs(canvas))
        if stones is None:
            return
        self.discard_lonelies(stones, reference=refs)
        if self.verify(self.sf.routine_constr[self.finder], stones, refs, img, id_="routine") < 0:
            return
        history = self.accus[self.finder]
        history[:] = self._inside(stones)
        self.commit(history)

    def try_clustering(self, img, refs, clustered=_UNSET):
        """score k-means on this region; verified results are committed even while another finder is in charge; when a
        cycle of scores is complete and not negative in sum, k-means takes the region over"""
        stones = self._clustered(img, clustered)
        checks = (self.sf.check_thickness, self.sf.check_against, self.sf.check_lines)
        score = -1 if stones is None else self.verify(checks, stones, refs, img, id_="tryclust")
        self.cluster_score[0] = score
        if score > 0:
            history = self.cluster_accu
            history[:] = self._inside(stones)
            self.commit(history)
        cycle_done = self.cluster_score.at_end()
        if cycle_done:
            total = int(np.sum(self.cluster_score.buffer))
            if total >= 0:
                self.finder = self.sf.cluster
                self._search_all()                          # a new finder runs a full cycle
                if total == 0 and int(np.max(self.cluster_score.buffer)) == 0:
                    print("Wild assignment of clustering to region {}".format((self.re, self.ce)))
        self.cluster_score.increment()
        self.population = self.get_population(refs)         # (the WHOLE goban's, as in the reference: sf_meta.py:274)

    def verify(self, constraints, stones, refs, img, id_=""):
        """-> the sum of the constraints' scores, or -1 as soon as one of them refuses"""
        total = 0
        for check in constraints:
            score = check(stones, img=img, reference=refs, rs=self.rs, re=self.re, cs=self.cs, ce=self.ce)
            if score < 0:
                print("{}{} vetoed region {}".format(id_ + ": " if id_ else "", getattr(check, "__name__", check), (self.re, self.ce)))
                return -1
            total += score
        return total

    def commit(self, cb):
        """submit what recurs in the history `cb`, where the goban is still empty: a colour seen together with E while E
        fills less than 40 % of the history, or a colour seen alone; then move the history on"""
        assert cb.buffer.ndim == 3
        moves = []
        for i, j in np.ndindex(cb.buffer.shape[:2]):
            r, c = i + self.rs, j + self.cs
            if not self.sf.is_empty(r, c):
                continue
            seen = list(cb.buffer[i, j])
            colours = sorted(set(seen))
            if len(colours) == 2 and E in colours:
                if seen.count(E) / cb.size < 0.4:
                    moves.append((colours[0] if colours[1] == E else colours[1], r, c))
            elif len(colours) == 1 and colours[0] != E:
                moves.append((colours[0], r, c))
        try:
            if len(moves) > 1:
                self.sf.bulk_update(moves)
            elif moves:
                self.sf.suggest(*moves[0], doprint=False)
        except DeletedError as locked:                      # (to be learnt from, some day)
            print(str(locked))
        cb.increment()

    # ---- foreground ------------------------------------------------------------------------------------------------------
    def check_foreground(self):
        """-> True when the region is calm.  The zones just outside the region are watched closely -- a disturbance there
        usually belongs to something bigger next door: two of them more than 70 % foreground, or one at a corner of the
        image, and the region is agitated.  Inside, up to three stones' worth of foreground is let through."""
        try:
            fg = self.sf.get_foreground()
        except ValueError:
            return True
        if fg is None:                                      # no background model: every frame counts as calm
            return True
        calm = self._border_calm(fg)
        if calm:
            x0, y0, x1, y1 = self.get_img_bounds()
            calm = not 3 * self.sf.stone_radius() ** 2 * math.pi < np.sum(fg[x0:x1, y0:y1]) / 255
        if not calm:
            self.set_agitated()
        return calm

    def _border_calm(self, fg):
        moving, enough = 0, 2
        for a0, b0, a1, b1 in self.outer_border():
            if (a1 - a0) * (b1 - b0) * 0.7 < np.sum(fg[a0:a1, b0:b1]) / 255:
                if (a0 == 0 or a1 == fg.shape[0] - 1) and (b0 == 0 or b1 == fg.shape[1] - 1):
                    moving = enough
                moving += 1
                if enough <= moving:
                    return False
        return True

    def _search_all(self):
        self.states.buffer[:] = Search

    def set_agitated(self):
        if self.states[0] == Warmup:
            self.states.replace(Idle, Warmup)               # (finds no idle slot while the current one is warmup; kept)
        else:
            self._search_all()

    def clustering_needs_try(self, ref_stones):
        now = self.get_population(self._inside(ref_stones))
        if now < 4:
            return False
        if not self.cluster_score.at_start():               # a cycle of tries has begun: finish it
            return True
        return self.finder is not self.sf.cluster and self.population + 1 < now

    def get_population(self, stones):
        return int(np.count_nonzero(np.asarray(stones, dtype=object) != E))

    def get_img_bounds(self):
        first, last = self.sf.getrect(self.rs, self.cs), self.sf.getrect(self.re - 1, self.ce - 1)
        return first[0], first[1], last[2], last[3]

    def discard_lonelies(self, stones, reference):
        """a first-line stone with nothing within two lines of it is not a move: taken out of `stones`, in place"""
        alone = self.sf.first_line_lonelies(stones, reference, rs=self.rs, re=self.re, cs=self.cs, ce=self.ce)
        for r, c in alone:
            stones[r, c] = E
        if len(alone):
            print("Discarded lonely stone(s) on first line {}".format(alone))

    def outer_border(self):
        """the zones around the region, outside it, clipped to the goban: down the left side, along the bottom, up the right
        side, back along the top"""
        last = gsize - 1
        col = max(0, self.cs - 1)
        for row in range(max(0, self.rs - 1), min(gsize, self.re + 1)):
            yield self.sf.getrect(row, col)
        row = min(last, self.re)
        for col in range(max(1, self.cs), min(gsize, self.ce + 1)):
            yield self.sf.getrect(row, col)
        col = min(last, self.ce)
        for row in range(min(last - 1, self.re - 1), max(-1, self.rs - 2), -1):
            yield self.sf.getrect(row, col)
        row = max(0, self.rs - 1)
        for col in range(min(last - 1, self.ce - 1), max(0, self.cs - 1), -1):
            yield self.sf.getrect(row, col)
