"""K9 (MOG2) on the CPU oracle, through the branches the GPU parity tests barely reach: the scenes of
tests/mog2_scenes.py held to floors on the oracle's own event counters, the oracle against the list-of-modes
restatement (saturation, the automatic rate through its cap, rate 0, a reset, rates of 0.6 .. 0.95), the update that
prunes every mode, and the prune bookkeeping of the ghost-mode sequence, pinned as it behaves today."""
import numpy as np
import pytest

from tests import mog2_scenes as S

# (scene, schedule, frames, {event: floor}) -- each scene must reach its events at least this often on 16 x 16 pixels
# (the floors are about half of what the scenes reach today)
FLOORS = [
    ("cycle", "0.01", 60, dict(new_mode=2000, replace=1500, bubble=2000)),
    ("cycle", "high", 80, dict(zero_total=150, prune_inner=300, prune=700)),
    ("noise", "auto", 260, dict(var_min=10000, var_max=500)),
    ("ghost", "0.2", 70, dict(prune=256)),                      # every pixel's transient mode, once
    ("hand", "0.3", 120, dict(prune=200, bubble=400)),
    ("tie", "tie", 40, dict(bubble=16 * 16 * 27)),             # every pixel, every rate-0 frame but the first
]


def _rates(schedule, n):
    try:
        return np.full(n, float(schedule))
    except ValueError:
        return S.rates(schedule, n)


def _assert_live_finite(state, what):
    vals = S.live_values(state)
    assert np.isfinite(vals).all(), "%s: %d non-finite live values" % (what, int((~np.isfinite(vals)).sum()))


def test_scene_event_floors(ora):
    """each scene reaches the branch it was built for (counted by the oracle), and no frame leaves a NaN / inf in a live
    slot (a poisoned mode can be evicted by a later replacement, so the check is after every frame)"""
    seen = dict.fromkeys(ora.MOG2_EVENTS, 0)
    for scene, schedule, n, floors in FLOORS:
        m = ora.MOG2(16, 16, 3)
        gen = S.tie if scene == "tie" else S.SCENES[scene]
        for t, (img, lr) in enumerate(zip(gen(16, 16, range(n), seed=3), _rates(schedule, n))):
            m.apply(img, lr)
            _assert_live_finite(m.state(), "%s at %s, frame %d" % (scene, schedule, t))
        ev = m.events()
        print("%-6s %-6s %s" % (scene, schedule, " ".join("%s=%d" % kv for kv in ev.items() if kv[1])))
        for k, v in ev.items():
            seen[k] += v
        for k, floor in floors.items():
            assert ev[k] >= floor, "%s at %s: %s reached %d times, floor %d" % (scene, schedule, k, ev[k], floor)
    print("all scenes:", " ".join("%s=%d" % kv for kv in seen.items()))
    assert all(v > 0 for v in seen.values()), seen


# crops of <= 16 x 16 pixels and <= 300 frames: the restatement is pure Python
CASES = [
    ("saturation", "cycle", 8, 8, "0.01", 60),
    ("auto-cap", "noise", 4, 6, "auto", 260),
    ("rate-zero", "mosaic", 8, 8, "zero", 80),
    ("reset", "mosaic", 8, 8, "reset", 80),
    ("high", "cycle", 8, 8, "high", 80),
    ("mixed", "mosaic", 8, 12, "mixed", 120),
    ("ghost", "ghost", 3, 3, "0.2", 70),
    ("hand", "hand", 9, 9, "0.3", 120),
    ("tie", "tie", 4, 4, "tie", 40),
]


@pytest.mark.parametrize("name,scene,h,w,schedule,n", CASES, ids=[c[0] for c in CASES])
def test_oracle_vs_list_restatement(ora, name, scene, h, w, schedule, n):
    """the C oracle against the list-of-modes statement of tests/mog2_scenes.py: every mask, and the whole mixture at
    the end (nmodes, then weight / variance / mean of the live slots bit for bit)"""
    gen = dict(S.SCENES, mosaic=S.mosaic, tie=S.tie)[scene]
    frames = gen(h, w, range(n), seed=11)
    r = _rates(schedule, n)
    want, want_state = S.reference(frames, r, return_state=True)
    m = ora.MOG2(h, w, 3)
    for t in range(n):
        assert np.array_equal(m.apply(frames[t], r[t]), want[t]), (name, t)
    bad = S.state_mismatch(m.state(), want_state)
    assert bad is None, bad
    if schedule == "auto":
        assert n > 250                                           # through the cap at 1 / 500


def test_all_pruned_update_keeps_the_mixture_finite(ora):
    """a pixel that matches none of its modes at a learning rate of ~0.67 or more has every mode pruned in one update:
    totalWeight is 0 and the renormalisation is skipped (1 / 0 = inf, and 0 * inf would write NaN into the surviving
    slots for good).  After the update the new colour's mode holds alpha, the pruned slots still inside the bound hold
    0, and the masks of the frames after it are the ones the guarded rule predicts."""
    h, w = 4, 4
    cyc = S.cycle(h, w, range(81), seed=5)
    new = np.full((1, h, w, 3), 77, np.uint8)                   # a colour none of the 5 modes holds
    frames = np.concatenate([cyc[:60], new, cyc[60:]])
    r = np.full(len(frames), 0.01)
    r[60] = 0.95
    m = ora.MOG2(h, w, 3)
    for t in range(60):
        m.apply(frames[t], r[t])
    before = m.state()
    assert (before["nmodes"] == 5).all()                         # saturated
    m.apply(frames[60], r[60])
    after = m.state()
    assert m.events()["zero_total"] == h * w                     # every pixel took the all-pruned path
    _assert_live_finite(after, "after the all-pruned update")
    for px in range(h * w):
        k = int(after["nmodes"][px])
        assert k >= 2
        assert after["weight"][0, px] == np.float32(0.95) and after["variance"][0, px] == 15
        assert (after["mean"][0, :, px] == 77).all()
        assert (after["weight"][1:k, px] == 0).all()
    want, want_state = S.reference(frames, r, return_state=True)
    for t in range(61, len(frames)):
        assert np.array_equal(m.apply(frames[t], r[t]), want[t]), t
    _assert_live_finite(m.state(), "at the end")
    bad = S.state_mismatch(m.state(), want_state)
    assert bad is None, bad


def test_ghost_mode_prune_shrinks_the_mode_count(ora):
    """Pins the prune bookkeeping (ASSUMPTION 2 of oracle/ora_mog2.c) as it behaves today.

    Ghost scene at rate 0.2: a background, a transient colour for 12 frames, 32 quiet frames in which the transient's
    mode decays below alpha * 0.05 and is pruned, then the same colour again.  Here a prune shortens the loop bound and
    the count stays shortened (nmodes = bound), so in the gap every pixel is back to ONE mode -- the assertion marked
    below.  Under the other bookkeeping (nmodes = nNewModes after the renormalisation, as the library is believed to
    do: VERDICT "What's weak" 2) the count would not shrink: the pruned mode would stay as a zero-weight ghost with
    its old mean and variance, that assertion would see 2, and on the colour's return the ghost would be revived with
    its old variance instead of a new mode opened at varInit 15.  A change of the bookkeeping flips exactly that
    assertion; the masks below come from the same rule in the list restatement and would move with it."""
    h, w, n = 3, 3, 70
    frames = S.ghost(h, w, range(n), seed=2)
    m = ora.MOG2(h, w, 3)
    trace = []
    for t in range(n):
        m.apply(frames[t], 0.2)
        trace.append((m.state()["nmodes"].copy(), m.events()["prune"]))
    assert trace[20][1] == 0 and (trace[20][0] == 2).all()      # background + transient, nothing pruned yet
    assert trace[51][1] == h * w                                 # one prune per pixel in the gap
    assert (trace[51][0] == 1).all()                             # <- the bookkeeping: nNewModes would leave 2 here
    assert (trace[60][0] == 2).all()                             # the colour is back, as a mode again
    want = S.reference(frames, np.full(n, 0.2))
    m2 = ora.MOG2(h, w, 3)
    for t in range(n):
        assert np.array_equal(m2.apply(frames[t], 0.2), want[t]), t
