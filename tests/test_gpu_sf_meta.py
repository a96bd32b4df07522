"""SfMeta on the library: a filmed synthetic game through BoardFinderAuto + SfMeta on the GPU, against the same finder over the
CPU stub (tests/cluster_ref.ClusterRefCtx: k-means from the plain reference, contour analysis and grid lines from the
oracle) fed the very goban images and foreground masks the GPU run produced.  The sequence of controller instructions must
be equal call by call, and so must the generator's state at the end: every random number was drawn in the same place.

How many of the filmed stones SfMeta finds is printed, not asserted (docs/lab_notes.md): the reference's author calls the
method unfinished (stone/sf_meta.py:22-23) and no figure for it exists."""
import types

import numpy as np
import pytest

from tests.test_sf_meta_cpu import Recorder

pytestmark = pytest.mark.gpu


def test_film_gives_the_same_instructions_as_the_cpu_stub(ora):
    from camkifu_amd import synth
    from camkifu_amd.core.vmanager import VManagerSeq
    from camkifu_amd.golib_shim import E
    from camkifu_amd.stone.sf_meta import SfMeta
    from tests.cluster_ref import ClusterRefCtx

    seen = []

    class Watched(SfMeta):
        def _find(self, goban_img):
            seen.append((np.array(goban_img), None if self.get_foreground() is None else np.array(self.get_foreground()),
                         self.total_f_processed))
            super()._find(goban_img)

    film, corners, truth, moves, hands = synth.film(84, 480, 640, seed=synth.SEED, density=0.3, quiet=62, move_every=10, hand_frames=4)
    ctrl = Recorder(video=film.numpy())
    vm = VManagerSeq(ctrl, sf="SfMeta")
    assert vm.sf_class is SfMeta and vm.bf_class.__name__ == "BoardFinderAuto"
    vm.sf_class = Watched
    vm.run()
    assert getattr(vm, "error", None) is None
    gpu = vm.stones_finder
    assert len(seen) > gpu.bg_init_frames + 10

    # the same frames through the finder over the CPU stub
    stub = ClusterRefCtx()
    ctrl2 = Recorder()
    cpu = SfMeta(types.SimpleNamespace(controller=ctrl2, device=0, current_video=None, imqueue=None), ctx=stub)
    for goban, fg, count in seen:
        cpu.goban_img, cpu._fg, cpu.intersections, cpu.total_f_processed = goban, fg, None, count
        cpu._learn()
        cpu._find(goban)
    assert len(ctrl.calls) == len(ctrl2.calls)
    for k, (a, b) in enumerate(zip(ctrl.calls, ctrl2.calls)):
        assert a == b, k
    assert gpu.ctx.rng_state == stub.rng_state and len(stub.cluster_calls) >= 1
    assert [r.states.buffer.tolist() for r in gpu.regions.flat] == [r.states.buffer.tolist() for r in cpu.regions.flat]
    assert [r.finder is gpu.cluster for r in gpu.regions.flat] == [r.finder is cpu.cluster for r in cpu.regions.flat]

    got, final = ctrl.get_stones(), truth[-1]
    right = sum(1 for r in range(19) for c in range(19) if got[r, c] != E and got[r, c] == "EBW"[final[r, c]])
    wrong = int((got != E).sum()) - right
    played = sum(1 for colour, r, c, f in moves if got[r, c] == "EBW"[colour])
    print("SfMeta on the film (GPU): %d stones submitted, %d right, %d wrong, of %d on the board; %d of %d filmed moves found; "
          "%d k-means calls, %d regions on k-means at the end"
          % (right + wrong, right, wrong, int((final > 0).sum()), played, len(moves), len(stub.cluster_calls),
             sum(r.finder is gpu.cluster for r in gpu.regions.flat)))
    assert right >= 1
    gpu.ctx.close()
