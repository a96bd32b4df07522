"""Standalone protocol base of a stones finder: the straightened goban image, the background model, the result
sink and the grid geometry a finder builds on (contract: reference stone/stonesfinder.py:95-176, 250-349,
412-450, 950-981).

    frame --K8 ck_warp_perspective(board_finder.mtx)--> goban_img 380x380x3
          --K9 ck_mog2_apply--> foreground mask --> _learn() (user corrections) --> _find(goban_img)

Pieces, each usable on its own (the batch pipeline's fold uses the sink without a finder):
    PosGrid        pixel position of the 361 intersections, and the zone (rectangle) around each as one table
    DeletionWatch  intersections the user emptied: averaged appearance, refusal of new stones until it changes
    StoneSink      (colour, row, col) decisions -> controller instructions "append" / "delete" / "bulk" / "auto_save"
    StonesFinder   the per-frame protocol: _doframe, ready_to_read, _find (abstract), suggest / remove / bulk_update,
                   getrect, get_foreground, corrected, is_empty, get_stones
Coordinates handed to suggest / remove / bulk_update are numpy (row, col)."""
import queue

import numpy as np

from .. import capi, cvconf
from ..core import imgutil, overlay
from ..core.exceptions import CorrectionWarning, DeletedError
from ..core.video import VidProcessor
from ..golib_shim import gsize, E, B, W, Move, NP_TYPE

correc_size = 10
_CODE = {E: 0, B: 1, W: 2}


class PosGrid:
    """`mtx[i, j]` = (x, y) pixel of intersection (i, j) in the canonical image: cell centres, 10 + 20 k at the
    default size.  `zones(cursor)` is the (19, 19, 4) table of rectangles (x0, y0, x1, y1) the reference computes one
    at a time in StonesFinder.getrect: bounded halfway (cursor 1.0) towards the diagonal neighbours, mirrored at the
    first line, stopping one pixel short of the image at the last."""

    def __init__(self, size):
        self.size = size
        half = size / gsize / 2
        line = (half * (gsize - 1 - np.arange(gsize)) + (size - half) * np.arange(gsize)) / (gsize - 1)
        self.mtx = np.stack(np.meshgrid(line, line, indexing="ij"), -1).astype(np.int16)
        self.adjust_vect, self.adjust_contribs = np.zeros(2, np.float32), 0
        self._zones = {}

    def zones(self, cursor=1.0):
        key = (float(cursor), self.mtx.tobytes())
        hit = self._zones.get(key)
        if hit is None:
            p = self.mtx.astype(np.int16)
            before = np.roll(p, (1, 1), (0, 1)).copy()                       # mtx[r - 1, c - 1] (index -1 wraps, as in Python)
            after = p[np.minimum(np.arange(gsize) + 1, gsize - 1)][:, np.minimum(np.arange(gsize) + 1, gsize - 1)].copy()
            before[0, :, 0] = -p[0, :, 0]
            before[:, 0, 1] = -p[:, 0, 1]
            after[-1, :, 0] = 2 * self.size - p[-1, :, 0] - 2
            after[:, -1, 1] = 2 * self.size - p[:, -1, 1] - 2
            k = 0.5 * cursor
            lo = np.maximum(0, (k * before + (1 - k) * p).astype(np.int64))  # astype truncates toward zero like int()
            hi = np.minimum(self.size, ((1 - k) * p + k * after).astype(np.int64))
            hit = np.concatenate([lo, hi], -1)
            self._zones = {key: hit}
        return hit

    def learn(self, grid, rate=0.2):
        """Drift correction (reference stonesfinder.py:1015-1043): `grid` is an updated copy of mtx (find_intersections'
        answer, made positive); the mean displacement of the intersections that moved is blended into `adjust_vect` at
        `rate`, and once more than 20 intersections have contributed the whole grid is shifted by it (truncated)."""
        if not 0 < rate <= 1:
            raise AssertionError("rate must lie in ]0, 1]")
        shift = np.asarray(grid, np.int16) - self.mtx
        if shift.min() < -200:
            raise ValueError("Provided grid seems too far from original, at least for one point.")
        movers = int(np.count_nonzero((shift != 0).any(-1)))
        if not movers:
            return
        step = shift.sum(axis=(0, 1), dtype=np.float32)
        step /= movers
        keep = 1.0 - rate
        self.adjust_vect *= keep                                   # float32 in place, as the reference's accumulator
        self.adjust_vect += step * rate
        self.adjust_contribs += movers
        if self.adjust_contribs <= 20:
            return
        whole = self.adjust_vect.astype(np.int16)                   # truncated toward zero
        print("Grid adjust vector : %s" % self.adjust_vect)
        self.mtx += whole
        self.adjust_vect.fill(0)
        self.adjust_contribs = 0


class DeletionWatch:
    """The user took a stone off (or moved it): that intersection is watched.  Over the next `samples` frames in which
    its zone is not entirely foreground the zone's pixels are averaged; from then on a stone is only accepted there
    once the zone differs from that average by 40 grey levels per pixel (all channels summed).
    reference: stonesfinder.py:178-245."""

    def __init__(self, shape, samples=50):
        self.samples = samples
        self.left = np.full((gsize, gsize), -1, np.int32)        # frames still to sample; -1 = not watched
        self.saved_bg = np.zeros(tuple(shape) + (3,), np.float32)

    def start(self, r, c):
        self.left[r, c] = self.samples

    def watched(self):
        return {(int(r), int(c)): int(self.left[r, c]) for r, c in np.argwhere(self.left >= 0)}

    def sample(self, goban_img, fg, zones):
        for r, c in np.argwhere(self.left > 0):
            x0, y0, x1, y1 = zones[r, c]
            # reference quirk kept: `np.sum(fg[zone] < 0.1 * area)` counts the pixels BELOW the bound, so the zone is
            # sampled as soon as one of its pixels is background
            if fg is None or (fg[x0:x1, y0:y1] < 0.1 * (x1 - x0) * (y1 - y0)).any():
                self.saved_bg[x0:x1, y0:y1] += goban_img[x0:x1, y0:y1] / self.samples
                self.left[r, c] -= 1

    def check(self, r, c, goban_img, zones):
        """raises DeletedError while (r, c) is locked; forgets the watch once the zone has changed enough"""
        state = self.left[r, c]
        if state < 0:
            return
        if state > 0:
            raise DeletedError(((r, c),), "The zone has been marked as deleted too recently.")
        x0, y0, x1, y1 = zones[r, c]
        delta = self.saved_bg[x0:x1, y0:y1] - goban_img[x0:x1, y0:y1]
        if np.sum(np.absolute(delta)) / (delta.shape[0] * delta.shape[1]) < 40:
            raise DeletedError(((r, c),), "The zone has not changed enough since last deletion.")
        print("intersection %s looks different from when the user emptied it: unlocked" % ((r, c),))
        self.left[r, c] = -1


class StoneSink:
    """What a finder decides -> what the controller is told.  `guard(r, c)` may raise DeletedError to veto a stone."""

    def __init__(self, controller_of, guard=None):
        self._controller_of, self._guard = controller_of, guard

    @property
    def controller(self):
        return self._controller_of()

    def is_empty(self, r, c):
        return self.controller.is_empty_blocking(c, r)

    def get_stones(self):
        return self.controller.get_stones()

    def board_codes(self):
        """the goban as uint8 (19, 19): 0 empty, 1 black, 2 white"""
        stones = self.get_stones()
        return (stones == B).astype(np.uint8) + 2 * (stones == W).astype(np.uint8)

    def _vet(self, r, c):
        if self._guard is not None:
            self._guard(r, c)

    def suggest(self, color, r, c, doprint=True):
        self._vet(r, c)
        stone = Move(NP_TYPE, (color, r, c))
        if doprint:
            print(stone)
        ctl = self.controller
        ctl.pipe("append", stone)
        ctl.pipe("auto_save")

    def remove(self, r, c):
        if self.is_empty(r, c):
            raise AssertionError("Can't remove stone from empty intersection.")
        gone = Move(NP_TYPE, ("", r, c))
        self.controller.pipe("delete", gone.x, gone.y)

    def bulk_update(self, tuples):
        """several changes as ONE controller instruction: E empties, B / W places (recolouring = empty, then place;
        an identical stone already there is skipped).  Vetoed places are left out and reported together afterwards.
        The goban is looked at as it WILL be after the changes already scheduled in this call, so a point named twice
        -- the regions of rows / columns 16-17 and 17-18 overlap and may both report it -- is sent once (or, if they
        disagree, settled in favour of the later one) instead of reaching the controller as two stones on one point."""
        ctl, batch, refused, scheduled = self.controller, [], [], {}

        def colour_at(r, c):
            if (r, c) in scheduled:
                return scheduled[(r, c)]
            return E if self.is_empty(r, c) else ctl.locate(c, r).color
        for color, r, c in tuples:
            now = colour_at(r, c)
            if color == E:
                if now != E:
                    batch.append(Move(NP_TYPE, (E, r, c)))
                    scheduled[(r, c)] = E
                continue
            if color not in (B, W) or now == color:
                continue
            if now != E:
                batch.append(Move(NP_TYPE, (E, r, c)))               # the clearing half goes out even if the stone is vetoed
                scheduled[(r, c)] = E
            try:
                self._vet(r, c)
            except DeletedError as veto:
                refused.append(veto)
                continue
            batch.append(Move(NP_TYPE, (color, r, c)))
            scheduled[(r, c)] = color
        if batch:
            ctl.pipe("bulk", batch)
            ctl.pipe("auto_save")
        if refused:
            raise DeletedError(refused, message="Bulk_update:warning: All non-conflicting locations have been sent.")


class StonesFinder(VidProcessor):
    def __init__(self, manager, learn_bg=True, ctx=None):
        VidProcessor.__init__(self, manager)
        self.ctx = ctx if ctx is not None else capi.Context(getattr(manager, "device", 0))
        side = cvconf.canonical_size
        self.canonical_shape, self.goban_img, self.intersections, self._fg = (side, side), None, None, None
        self._posgrid = PosGrid(side)
        self.watch = DeletionWatch(self.canonical_shape)
        self.corrections = queue.Queue(correc_size)
        self.sink = StoneSink(lambda: self.vmanager.controller, self._check_dels)
        if learn_bg:
            self.bg_model = self.ctx.mog2_create(side, side)
            video = getattr(manager, "current_video", None)
            still = isinstance(video, str) and video.lower().endswith((".png", ".jpg"))
            self.bg_init_frames = 0 if still else 50

    # ---- per frame -------------------------------------------------------------------------------
    def ready_to_read(self):
        bf = getattr(self.vmanager, "board_finder", None)
        return VidProcessor.ready_to_read(self) and getattr(bf, "mtx", None) is not None

    def _doframe(self, frame):
        bf, self.intersections = self.vmanager.board_finder, None
        mtx = None if bf is None else bf.mtx
        if mtx is None:
            return
        goban = self.goban_img = self.ctx.warp_perspective(frame, mtx, cvconf.canonical_size)   # K8
        for stage in (self._learn_bg, self._learn):
            stage()
        self._find(goban)

    def _find(self, goban_img):
        raise NotImplementedError("a stones finder implements _find(goban_img)")

    def _learn_bg(self):
        if getattr(self, "bg_model", None) is not None:
            rate = 0.01 if self.total_f_processed < self.bg_init_frames else 0.005
            self._fg = self.ctx.mog2_apply(self.bg_model, self.goban_img, rate)                  # K9

    def get_foreground(self):
        return self._fg

    # ---- empty intersections from grid lines ----------------------------------
    def find_intersections(self, img, canvas=None):
        """Which intersections show grid lines, hence no stone (reference stonesfinder.py:516-552): one library call
        (ck_find_intersections: grey / Otsu / Canny and one HoughLinesP wave per zone on the GPU, update_grid on the
        host) -> a copy of the grid with the positions where a line was found negated, and moved where a cross was.
        `canvas` (the reference's drawing surface) is accepted and left alone."""
        return self.ctx.find_intersections(np.ascontiguousarray(img, np.uint8), self._posgrid.mtx, self._posgrid.zones(1.0))

    def get_intersections(self, img, display=False):
        """cached per frame (reset in _doframe); the grid learns from every fresh answer (stonesfinder.py:554-576)"""
        cached = self.intersections
        if cached is None:
            cached = self.intersections = self.find_intersections(img)
            self._posgrid.learn(np.abs(cached))
        return cached

    # ---- consistency checks on a candidate result (stonesfinder.py:597-783; vectorised in stone/checks.py) ---------
    def check_against(self, stones, reference=None, rs=0, re=gsize, cs=0, ce=gsize, **kwargs):
        from . import checks
        return checks.check_against(stones, reference, rs, re, cs, ce)

    def check_lines(self, stones, img=None, rs=0, re=gsize, cs=0, ce=gsize, **kwargs):
        from . import checks
        return checks.check_lines(stones, self.get_intersections(img), rs, re, cs, ce)

    def check_thickness(self, stones, rs=0, re=gsize, cs=0, ce=gsize, **kwargs):
        from . import checks
        return checks.check_thickness(stones, rs, re, cs, ce)

    def check_flow(self, stones, rs=0, re=gsize, cs=0, ce=gsize, **kwargs):
        from . import checks
        return checks.check_flow(stones, self.sink.board_codes().reshape(gsize, gsize) == 0, rs, re, cs, ce)

    def first_line_lonelies(self, stones, reference=None, rs=0, re=gsize, cs=0, ce=gsize, **kwargs):
        from . import checks
        return checks.first_line_lonelies(stones, reference, rs, re, cs, ce)

    # ---- user corrections ------------------------------------------------------------------------
    def corrected(self, err_move, exp_move):
        pending = self.corrections
        try:
            pending.put_nowait((err_move, exp_move))
        except queue.Full:
            print("Corrections queue full (%s), ignoring %s -> %s" % (correc_size, err_move, exp_move))

    def _learn(self):
        """drain the corrections: a deletion (or the origin of a moved stone) goes under watch; anything else cannot be
        learnt from here and is reported (CorrectionWarning) after this frame's sampling"""
        leftover = []
        while True:
            try:
                wrong, right = self.corrections.get_nowait()
            except queue.Empty:
                break
            moved = wrong is not None and right is not None and (wrong.x, wrong.y) != (right.x, right.y)
            if right is None or moved:
                self.watch.start(wrong.y, wrong.x)                 # Move.x is the column, Move.y the row
            else:
                leftover.append((wrong, right))
        self.watch.sample(self.goban_img, self.get_foreground(), self._posgrid.zones())
        if leftover:
            raise CorrectionWarning(leftover, message="Unhandled corrections")

    def _check_dels(self, r, c):
        self.watch.check(r, c, self.goban_img, self._posgrid.zones())

    @property
    def deleted(self):
        return self.watch.watched()

    @property
    def saved_bg(self):
        return self.watch.saved_bg

    @property
    def nb_del_samples(self):
        return self.watch.samples

    @nb_del_samples.setter
    def nb_del_samples(self, n):
        self.watch.samples = n

    # ---- results ---------------------------------------------------------------------------------
    def suggest(self, color, r, c, doprint=True):
        self.sink.suggest(color, r, c, doprint)

    def remove(self, r, c):
        self.sink.remove(r, c)

    def bulk_update(self, tuples):
        self.sink.bulk_update(tuples)

    def is_empty(self, r, c):
        return self.sink.is_empty(r, c)

    def get_stones(self):
        return self.sink.get_stones()

    # ---- geometry --------------------------------------------------------------------------------
    def getrect(self, r, c, cursor=1.0):
        if not isinstance(cursor, float):
            raise TypeError("cursor must be a float in ]0, 2[")
        return tuple(int(v) for v in self._posgrid.zones(cursor)[r, c])

    def stone_radius(self):
        """radius of a stone in the canonical image, in pixels (stonesfinder.py:578-584)"""
        return self._posgrid.size / gsize / 2

    def getmask(self, depth=1):
        """a disc around every intersection (stonesfinder.py:452-490): (side, side) uint8 of 0 / 1 -- (side, side, depth)
        for depth > 1 -- built from the zone table and kept until that table or `depth` changes.  Each zone holds the disc
        of radius min(h, w) / 2 about its centre; zones are written in raster order; pixels no zone covers are 0 (the
        reference leaves them uninitialised, and never reads them)."""
        zones = self._posgrid.zones(1.0)
        key = (zones.tobytes(), int(depth))
        cached = getattr(self, "_mask_cache", None)
        if cached is None or cached[0] != key:
            side = self._posgrid.size
            flat = np.zeros((side, side), np.uint8)
            for x0, y0, x1, y1 in zones.reshape(-1, 4):
                h, w = flat[x0:x1, y0:y1].shape
                dy = np.arange(h)[:, None] - h / 2
                dx = np.arange(w)[None, :] - w / 2
                flat[x0:x1, y0:y1] = dx * dx + dy * dy <= min(h / 2, w / 2) ** 2
            mask = flat if depth <= 1 else np.repeat(flat[:, :, None], depth, axis=2)
            cached = self._mask_cache = (key, mask)
        return cached[1]

    # ---- display: each builds ONE display list and makes one library call (core/overlay.py) ----------------------
    def _grid_list(self, into=None):
        dl = into if into is not None else overlay.DisplayList()
        if self._posgrid is not None:
            for p in self._posgrid.mtx.reshape(-1, 2):
                dl.circle(int(p[1]), int(p[0]), 5, (255, 255, 0))
        return dl

    def _drawgrid(self, img):
        """a circle of radius 5 in (255, 255, 0) around each intersection as currently estimated (reference
        stone/stonesfinder.py:786-790)"""
        overlay.draw(img, self._grid_list(), getattr(self, "ctx", None))

    def _drawvalues(self, img, values):
        """one value per goban position, str(value) at (x - 10, y + 2) of mtx[row, col] = (x, y) as the reference writes
        it (:801-806); None draws nothing"""
        dl = overlay.DisplayList()
        for row in range(gsize):
            for col in range(gsize):
                if values[row, col] is not None:
                    x, y = (int(v) for v in self._posgrid.mtx[row, col])
                    imgutil.str_list(img, str(values[row, col]), x - 10, y + 2, into=dl)
        overlay.draw(img, dl, getattr(self, "ctx", None))

    def draw_stones(self, stones, canvas=None):
        """an array of stones (gsize, gsize) as discs of radius 10, black (0, 0, 0) or white (255, 255, 255), on `canvas`
        -- default: a new brown one, (65, 100, 128) -- then the grid's circles (reference :823-837) -> canvas"""
        if canvas is None:
            canvas = np.zeros((self._posgrid.size, self._posgrid.size, 3), np.uint8)
            canvas[:] = (65, 100, 128)
        dl = overlay.DisplayList()
        for x in range(gsize):
            for y in range(gsize):
                if stones[x][y] == B or stones[x][y] == W:
                    p = self._posgrid.mtx[x][y]
                    dl.disc(int(p[1]), int(p[0]), 10, (0, 0, 0) if stones[x][y] == B else (255, 255, 255))
        overlay.draw(canvas, self._grid_list(dl), getattr(self, "ctx", None))
        return canvas

    def display_intersections(self, grid, img):
        """how the intersection analysis is doing (reference :852-860): a circle of radius 5 in get_display_color(i, j)
        at every intersection of `grid` (find_intersections' answer: negated positions), over a black one where the
        position was updated; then the image is shown.  cv2's even thicknesses 2 and 6 become the odd 3 and 7 of the
        rasteriser, which keep the radius in the middle of the band."""
        dl = overlay.DisplayList()
        for i in range(grid.shape[0]):
            for j in range(grid.shape[1]):
                inter = grid[i][j]
                dif = self._posgrid.mtx[i][j] + inter
                if 0 < abs(int(dif[0])) + abs(int(dif[1])):
                    dl.circle(-int(inter[1]), -int(inter[0]), 5, (0, 0, 0), thickness=7)
                dl.circle(-int(inter[1]), -int(inter[0]), 5, self.get_display_color(i, j), thickness=3)
        overlay.draw(img, dl, getattr(self, "ctx", None))
        self._show(img, "{} - Intersections".format(self._window_name()))

    @staticmethod
    def get_display_color(i, j):
        """the colour of intersection (i, j) in display_intersections (reference :866-870)"""
        factor = 0.5 if i % 2 else 1
        return 40 / factor, (230 if j % 2 else 10) * factor, (10 if j % 2 else 200) * factor

    def display_message(self, message, name=None, force=False):
        """a message in the middle of a black image of the goban image's shape (reference :883-885)"""
        black = np.zeros(self.goban_img.shape[0:2], np.uint8)
        imgutil.draw_str(black, message)
        self._show(black, name=name)

    def _window_name(self):
        return "camkifu.stone.stonesfinder.StonesFinder"


def update_grid(lines, box, result_slot):
    """reference stonesfinder.py:888-947, as a module function like there: the library's host routine"""
    capi.update_grid(lines, box, result_slot)
