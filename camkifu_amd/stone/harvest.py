"""Training data from a filmed game: the film and its SGF go through the fast-file pipeline once, and exactly those
classifier patches are kept whose label is certain.  The reference gets its datasets from snapshots that a person
validates in a window (core/vmanager.py:309-325, stone/nn_manager.py:133-214); at the rate the stones path runs here
that makes no sense, so the labels come from the game record instead, and the selection and the cut run on the GPU
where the goban images already lie (csrc/k_harvest.hip).

The labelling rule (label_windows).  For every processed frame f:
    G_f      the goban the finder has reported up to and including f (the fold's requests replayed on a controller)
    S_k      the reference game after k moves, k = 0 .. K (reference_positions: the same controller, the same `rules`)
    k_f      the smallest k >= the last matched k with G_f == S_k, else -1: a match is searched forward only
A window begins whenever k_f changes, and it is closed by the first frame one of whose zones has more than `agitation`
foreground pixels.  state_of[f] = k_f inside an open window with k_f >= 1, else -1.  Three guards:
    - state 0 never opens a window: before the finder has said anything G is trivially empty while the table is not;
    - a window ends at the first agitation: a hand, or a fresh stone that is still foreground, ends it, so the gap between
      "stone on the table" and "the finder has said so" is never harvested;
    - inside the kernel a region is taken only if the foreground counts of its four zones sum to <= calm_max.
A move the finder misses or misreads makes G stop matching any S_k: nothing further is harvested."""
import numpy as np

from ..controller import ControllerHeadless
from ..golib_shim import Kifu, Move, NP_TYPE, B, W
from .nn_manager import NB_CLASSES


def _codes(controller):
    stones = controller.get_stones()
    return (stones == B).astype(np.uint8) + 2 * (stones == W).astype(np.uint8)


def reference_positions(kifu, rules=False):
    """the game after 0, 1, .., K moves as (K + 1, 19, 19) uint8 codes 0 E / 1 B / 2 W.  kifu: a golib_shim.Kifu, the path of
    an SGF file, or a list of moves / (colour, row, col) tuples.  rules: captures leave the goban, as on a
    ControllerHeadless(rules=True)"""
    if isinstance(kifu, str):
        kifu = Kifu(kifu)
    moves = kifu.get_move_seq() if isinstance(kifu, Kifu) else list(kifu)
    ctrl = ControllerHeadless(rules=rules)
    out = [_codes(ctrl)]
    for mv in moves:
        if not isinstance(mv, Move):
            mv = Move(NP_TYPE, tuple(mv))
        ctrl.pipe("append", Move(NP_TYPE, (mv.color, mv.y, mv.x)))
        out.append(_codes(ctrl))
    return np.stack(out)


def replay(mirror, emitted):
    """the fold's per-frame requests, replayed on the controller `mirror` -> G_f of the frames (n, 19, 19)"""
    from .stonesfinder import StoneSink
    from ..capi import PolicyCore
    sink = StoneSink(lambda: mirror)
    out, now = np.empty((len(emitted), 19, 19), np.uint8), _codes(mirror)
    for f, requests in enumerate(emitted):
        for kind, moves in requests:
            if kind == PolicyCore.SUGGEST:
                sink.suggest(*moves[0], doprint=False)
            else:
                sink.bulk_update(moves)
        if requests:
            now = _codes(mirror)
        out[f] = now
    return out


def new_window_state():
    """what label_windows carries from one batch to the next"""
    return dict(last=0, k=0, closed=False)


def label_windows(found, fgcount, positions, agitation=200, state=None):
    """state_of (n,) int32 for n consecutive frames: found (n, 19, 19) = G_f, fgcount (n, 19, 19) or (n, 361) foreground
    counts, positions (K + 1, 19, 19) = S_k (module docstring).  Pure numpy.  state: new_window_state() of the film, updated
    in place, so that a film may come in batches; None: the frames are the start of a film"""
    st = new_window_state() if state is None else state
    found = np.asarray(found, np.uint8).reshape(-1, 361)
    positions = np.asarray(positions, np.uint8).reshape(-1, 361)
    agitated = np.asarray(fgcount).reshape(len(found), -1).max(axis=1) > agitation
    out = np.full(len(found), -1, np.int32)
    seen, k_f = None, -1
    for f in range(len(found)):
        if seen is None or not np.array_equal(found[f], seen):        # G changes on a few frames of a film only
            seen = found[f]
            hit = np.flatnonzero((positions[st["last"]:] == seen).all(axis=1))
            k_f = st["last"] + int(hit[0]) if len(hit) else -1
        if k_f >= 0:
            st["last"] = k_f
        if k_f != st["k"]:
            st["k"], st["closed"] = k_f, False
        if agitated[f]:
            st["closed"] = True
        if k_f >= 1 and not st["closed"]:
            out[f] = k_f
    return out


class Harvester:
    """A one-rank FastFilePipeline with its own ControllerHeadless that keeps, batch after batch, the patches of the frames
    label_windows lets through.  feed(frames) takes the next frames of the film (numpy, or a torch tensor in HBM),
    run(capture) a whole .y4m / .avi file or an array of frames, dataset() returns what has been gathered so far.
    Thinning: every `stride`-th eligible frame of a state, at most `per_state` frames per state; `empty_keep` of 256 empty
    regions are kept (a stateless hash of seed, frame and region), `calm_max` is the kernel's gate.  A context given as `ctx`
    classifies with the weights it holds; without one the process-wide context is used and given `net` (default: the
    current network, NNManager.get_net).  `pipe_args` go to the pipeline (bg_init_frames, ctx_board ...)."""

    def __init__(self, h, w, sgf, ctx=None, rules=False, per_state=None, stride=1, calm_max=16, empty_keep=256, seed=20161001,
                 agitation=200, net=None, **pipe_args):
        from .. import capi
        from ..pipeline import FastFilePipeline
        from .nn_manager import NNManager
        self.ctx = ctx if ctx is not None else capi.get_context()
        if ctx is None or net is not None:
            self.ctx.cnn_set_weights(NNManager.get_net() if net is None else net)
        self.positions = reference_positions(sgf, rules=rules)
        self.controller = ControllerHeadless(rules=rules)
        self._mirror = ControllerHeadless(rules=rules)                 # the requests replayed frame by frame: G_f
        harvester = self

        class _Pipe(FastFilePipeline):
            def process_batch(self, my_frames, n_total):
                emitted = FastFilePipeline.process_batch(self, my_frames, n_total)
                harvester._harvest(emitted, n_total)
                return emitted
        self.pipe = _Pipe(h, w, self.controller, ctx=self.ctx, keep_gobans=True, **pipe_args)
        self.per_state, self.stride = per_state, max(1, int(stride))
        self.calm_max, self.empty_keep, self.seed, self.agitation = int(calm_max), int(empty_keep), int(seed), agitation
        self.frames_seen = 0
        self.eligible = []                                             # (frame, state) of every frame label_windows let through
        self._window = new_window_state()
        self._seen, self._kept = {}, {}                                # per state: eligible frames met / frames harvested
        self._parts = []

    # ---- per batch -------------------------------------------------------------------------------------------
    def _replay(self, emitted):
        """the fold's per-frame requests -> G_f of the batch's frames (n, 19, 19)"""
        return replay(self._mirror, emitted)

    def _thin(self, state_of, first):
        out = state_of.copy()
        for f in np.flatnonzero(state_of >= 0):
            k = int(state_of[f])
            self.eligible.append((first + int(f), k))
            met, kept = self._seen.get(k, 0), self._kept.get(k, 0)
            self._seen[k] = met + 1
            if met % self.stride or (self.per_state is not None and kept >= self.per_state):
                out[f] = -1
            else:
                self._kept[k] = kept + 1
        return out

    def _harvest(self, emitted, n):
        first, self.frames_seen = self.frames_seen, self.frames_seen + n
        gobans, fg = self.pipe.last_gobans, self.pipe.last_fgcount
        found = self._replay(emitted)
        if gobans is None or fg is None:                               # no transform yet: nothing was warped
            return
        state_of = self._thin(label_windows(found, fg, self.positions, self.agitation, self._window), first)
        if not (state_of >= 0).any():
            return
        x, labels, src = self.ctx.harvest_patches(gobans, fg, state_of, self.positions, calm_max=self.calm_max,
                                                  empty_keep=self.empty_keep, seed=self.seed, first_frame=first)
        x, labels, src = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (x, labels, src))
        self._parts.append((x, labels, first + src[:, 0], src[:, 1], state_of[src[:, 0]]))

    # ---- entry points ------------------------------------------------------------------------------------------
    def feed(self, frames):
        """the next frames of the film, in order -> the requests the fold emitted for them"""
        return self.pipe.process_batch(frames, len(frames))

    def run(self, capture, batch=256, file_fps=None):
        """a whole film: the path of a .y4m / .avi file, an open capture of one, or an array of frames (n, h, w, 3).  A
        file's frames are selected as process_y4m selects them (file_frame_indices); of an array every frame is taken
        unless file_fps is given (the array then counts as a 30 fps film)"""
        from ..core.capture import AviMjpegCapture, Y4MCapture, file_frame_indices, open_capture
        if isinstance(capture, str):
            capture = open_capture(capture)
        if isinstance(capture, Y4MCapture):
            self.pipe.process_y4m(capture, batch=batch, file_fps=file_fps)
        elif isinstance(capture, AviMjpegCapture):
            self.pipe.process_mjpeg(capture, batch=batch, file_fps=file_fps)
        else:
            frames = getattr(capture, "frames", capture)
            if file_fps is not None:
                frames = frames[np.array(file_frame_indices(len(frames), 30.0, file_fps), np.int64)]
            for b0 in range(0, len(frames), batch):
                self.feed(frames[b0:b0 + batch])
        return self.dataset()

    def dataset(self):
        """dict(X uint8 (N, 40, 40, 3), Y bool (N, 81), frame (N,) = the processed frame's number, region (N,), state (N,) =
        the reference position the label was read from)"""
        if self._parts:
            x, labels, frame, region, state = (np.concatenate(col) for col in zip(*self._parts))
        else:
            x, labels = np.zeros((0, 40, 40, 3), np.uint8), np.zeros(0, np.uint8)
            frame = region = state = np.zeros(0, np.int64)
        y = np.zeros((len(labels), NB_CLASSES), bool)
        y[np.arange(len(labels)), labels] = True
        return dict(X=x, Y=y, frame=frame.astype(np.int64), region=region.astype(np.int32), state=state.astype(np.int32))

    def save(self, path):
        with open(path, "wb") as f:
            np.savez_compressed(f, **self.dataset())

    def close(self):
        self.pipe.close()
