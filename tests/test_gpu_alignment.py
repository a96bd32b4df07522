"""Every entry point on device pointers of any alignment.

A device tensor handed to capi.Context is taken as it lies, and torch's allocator hands out blocks on 512 bytes: apart from four
cases (test_ccl_unaligned_device_pointer, test_contours_external_from_an_unaligned_device_pointer, the narrow-form case of
tests/test_gpu_pyr.py and one jpeg_forward of tests/test_gpu_jpeg_enc.py) every GPU test of the suite gives the kernels pointers
on 16 bytes.  A caller who passes frames[1:], a row range of a byte buffer or a tensor out of a pool does not.  Here, with
tests/align_cases.py (placement inside one allocation, guard bands of 0x5A in front and behind):

  * every (method, argument) of tests/handover_cases.TURNS, and the frames of png_encode, lies in HBM at every offset of its element type, the others in
    host memory (in HBM at offset 0 where capi wants one memory space); then all device-capable arguments at the same offset
                                                                                  test_an_input_at_every_offset
  * every method with an `out=` parameter writes into an `out` at every offset, from inputs in host memory and from inputs in
    HBM at another offset                                                         test_an_out_at_every_offset
  * a placed record buffer is written at offsets 0 and 8 and refused at 4        test_record_rows_at_an_offset
  * the `edges` of ck_board_edges, ck_goban_canny and ck_canny, which capi allocates itself, at every offset through ctypes
                                                                                  test_the_edges_of_the_c_abi_at_every_offset

A run passes when its result passes the row's own check (tests/scratch_cases.py, tests/align_cases.py: the plain reference of
the method's own test file, never the library's host-memory answer), or when it is refused with CK_ERR_ARG and the message of
align_cases.ALLOWED for exactly that (method, argument, offset) -- and the same context then answers the aligned call.  An
entry of ALLOWED that is NOT refused fails as well: the table is what the library does, no more and no less.  After every run
the guard bands are untouched and the inputs hold what they held (overlay_draw and the record methods write in place: their
result is checked in the placed tensor).  The classifier rows go through all four modes on the exact network, stones_detect
and stones_run (the warp in front of it) included.

docs/lab_notes.md (note 19) goes through the guarded and the unguarded wide accesses one by one.

Mutants, each built as a library of its own, run once against this file on an MI355X, and not kept (only mutants whose wrong
store lands inside the guard band or the tensor itself; none that lets a wide access loose on an odd address):

  1 k_warp.hip: the byte-store tail of a row stored as whole dwords where the address allows (`dx0 + 3 < dsize` dropped
        from the guard at :99, the address test kept): at dsize 7 a thread with three pixels left writes twelve bytes
        -> test_an_out_at_every_offset[warp_perspective_dsize_7]: the three bytes too many are zeros on the next row's first
           pixel, written in a race with that row's own thread ("6 of 294 elements differ"); no other dsize of the file
           has a tail
  2 k_color.hip: the wide form's last dword of a row written one dword further on (`d4[x + 4 >= w ? 3 : 2]`)
        -> test_an_out_at_every_offset[i420_to_bgr]: "4 bytes of the guard band behind the tensor were written, the first
           at 0"; the row with `levels` goes through ck_i420_to_bgr_pyr, not this kernel, and the 6 x 10 row takes the narrow form
  3 k_jpeg.hip:224: the same in jpeg_reconstruct_kernel<S, true>
        -> test_an_out_at_every_offset[jpeg_reconstruct], [jpeg_decode_host], [jpeg_decode_device]: the band behind, 4 bytes;
           the 16 x 18 row takes the narrow form
  4 k_records.hip without its two refusals: seen by tests/test_gpu_arg_contract.py alone, run alone against it
        -> test_refused_with_its_code_and_message[board_records_rec_off_8], test_region_records_refuse_rows_off_8_bytes

Mutants 1 to 3 were run against test_an_out_at_every_offset only: there every store of theirs lands in the placed tensor or
its bands, while the input tests hand the kernels fresh torch blocks without bands.  Not once, as intended, but three times
each: the first run showed all three as wrong pixels, because the row's check (and a check of the host-memory run that gives
the output's shape) came before the band check; the order was changed twice, and the lines above are the third run's.  Mutant
4 was run once.

Found by reading, not by running: the NMS kernel of k_canny.hip chose its dword stores by `idx & 3`, the index, while `edges`
is the caller's device pointer in ck_board_edges, ck_goban_canny and ck_canny.  capi never lets a caller place it; a C caller
may.  The guard now takes the addresses in, and test_the_edges_of_the_c_abi_at_every_offset places `edges` (and ck_canny's
`map_out`) through ctypes at every offset."""
import numpy as np
import pytest

from tests import align_cases as ac
from tests import handover_cases as hc
from tests import scratch_cases as sc
from tests.align_cases import stops_at_a_hip_error

pytestmark = pytest.mark.gpu
ALLOWED = ac.ALLOWED


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def table(ck, ora):
    return ac.rows(ck, ora)


class Placer:
    """what a row's run gets as `place`: argument k goes to HBM at `offset` when its turn has come, to HBM at offset 0 when
    `others` says so, and stays in host memory otherwise; every placed tensor is kept for the checks after the call"""

    def __init__(self, method, turns, offset, others=False):
        self.method, self.turns, self.offset, self.others, self.seen = method, set(turns), offset, others, []

    def __call__(self, k, a):
        assert np.dtype(a.dtype) == np.dtype(ac.ARGS[self.method][k]), (self.method, k, a.dtype)
        if k not in self.turns and not self.others:
            return a
        t = ac.place(a, self.offset if k in self.turns else 0)
        self.seen.append((k, np.array(a, copy=True), t))
        return t

    def verify(self, placed_any=True):
        assert self.seen or not placed_any, "bad set-up: nothing was placed"
        for k, a, t in self.seen:
            ac.untouched(t)
            if (self.method, k) not in ac.IN_PLACE:
                ac.unchanged(t, a)


def _refused(err, fragments, what):
    from camkifu_amd import capi
    if getattr(err, "code", None) == capi.CK_ERR_HIP:
        raise err
    assert fragments, "%s was refused, and ALLOWED has no such entry: %s" % (what, err)
    assert getattr(err, "code", None) == capi.CK_ERR_ARG and any(f in str(err) for f in fragments), (what, str(err), fragments)


def _run_placed(ck, row, method, turns, offset, what):
    """one run of `row` with the arguments `turns` at `offset`: its check, or the refusal ALLOWED names"""
    from camkifu_amd import capi
    others = method in ac.ONE_SPACE
    fragments = [ALLOWED[(method, k, offset)] for k in sorted(turns) if (method, k, offset) in ALLOWED]
    p = Placer(method, turns, offset, others)
    try:
        got = row.run(ck, place=p)
    except capi.CkError as err:
        _refused(err, fragments, what)
        p.verify()
        again = Placer(method, turns, 0, others)                     # the same context answers the aligned call
        row.check(row.run(ck, place=again))
        again.verify()
        return
    assert not fragments, "%s is in ALLOWED and was not refused" % what
    p.verify()
    row.check(got)


INPUT_TURNS = list(ac.TURNS) + [(m, "all") for m in ac.METHODS if len(ac.ARGS[m]) > 1]


@pytest.mark.parametrize("method,turn", INPUT_TURNS, ids=["%s-%s" % t for t in INPUT_TURNS])
@stops_at_a_hip_error
def test_an_input_at_every_offset(ck, table, method, turn):
    n = len(ac.ARGS[method])
    turns, offsets = (range(n), ac.shared_offsets(method)) if turn == "all" else ([turn], ac.offsets_of(method, turn))
    from camkifu_amd import capi
    # the classifier's own rows go through the four modes themselves; the two that classify a warped frame do so here (the
    # exact network's answer is the same bits in every mode, so their check stays the one it is)
    modes = sc.MODES if method in ("stones_detect", "stones_run") else (None,)
    for name in ac.ROWS_OF[method]:
        row = table[name]
        if hasattr(row, "reaches"):
            row.reaches()
        for offset in offsets:
            for mode in modes:
                try:
                    if mode is not None:
                        ck.cnn_set_mode(sc._mode(mode))
                    _run_placed(ck, row, method, turns, offset, "%s, argument %s at offset %d%s" % (name, turn, offset, ", mode " + mode if mode else ""))
                finally:
                    ck.cnn_set_mode(capi.CK_CNN_DEFAULT)


def _input_offset(method, out_offset):
    """an offset for the inputs of an `out=` run: another one than the output's where the inputs may lie at another"""
    if method not in ac.ARGS:
        return None                                                  # (host streams: no device-capable argument)
    n = len(ac.ARGS[method])
    free = [o for o in ac.shared_offsets(method) if not any((method, k, o) in ALLOWED for k in range(n))]
    later = [o for o in free if o > out_offset] + [o for o in free if o < out_offset]
    return later[0] if later else free[0]


OUT_CASES = [(m, name) for m in ac.OUT for name in ac.OUT_ROWS[m]]


@pytest.mark.parametrize("method,name", OUT_CASES, ids=[c[1].replace(" ", "_") for c in OUT_CASES])
@stops_at_a_hip_error
def test_an_out_at_every_offset(ck, table, method, name):
    from camkifu_amd import capi
    row = table[name]
    first = row.run(ck)                                              # host memory: only the shape and the element type of the result
    zeros = np.zeros(first.shape, first.dtype)
    assert zeros.dtype == np.dtype(ac.OUT[method])
    n = len(ac.ARGS.get(method, ()))
    for offset in ac.offsets_of(method, "out"):
        for inputs in ("host", "device"):
            if (inputs == "host" and method in ac.OUT_NEEDS_DEVICE_INPUT) or (inputs == "device" and not n):
                continue
            what = "%s, out at offset %d, inputs in %s memory" % (name, offset, inputs)
            fragment = ALLOWED.get((method, "out", offset))

            p = Placer(method, range(n) if inputs == "device" else (), _input_offset(method, offset) if inputs == "device" else 0)
            out = ac.place(zeros, offset)
            try:
                got = row.run(ck, place=p if n else None, out=out)
            except capi.CkError as err:
                _refused(err, [fragment] if fragment else [], what)
                ac.untouched(out)
                ac.unchanged(out, zeros)                             # nothing was written
                p.verify(placed_any=inputs == "device")
                p = Placer(method, range(n) if inputs == "device" else (), 0)
                out = ac.place(zeros, 0)                             # the same context answers the aligned call
                got = row.run(ck, place=p if n else None, out=out)
            else:
                assert fragment is None, "%s is in ALLOWED and was not refused" % what
            assert got is out, what
            ac.untouched(out)                                        # (first: a store past the end says more than a wrong pixel)
            p.verify(placed_any=inputs == "device")
            row.check(got)


@pytest.mark.parametrize("offset", [0, 8, 4])
@pytest.mark.parametrize("method", ["board_detect_records", "cnn_regions_records"])
@stops_at_a_hip_error
def test_record_rows_at_an_offset(ck, table, method, offset):
    """the rows in HBM at offset 0 and at offset 8 are written, at offset 4 they are refused ("records must be 8-byte aligned")
    and stay as they were; the frames in host memory, then in HBM as well"""
    from camkifu_amd import capi
    row = table[method]
    for turns in ([1], [0, 1]):
        p = Placer(method, turns, offset)
        if offset % 8:
            with pytest.raises(capi.CkError, match="records must be 8-byte aligned") as err:
                row.run(ck, place=p)
            assert err.value.code == capi.CK_ERR_ARG
            for k, a, t in p.seen:
                ac.untouched(t)
                ac.unchanged(t, a)                                   # the refused rows too
        else:
            row.check(row.run(ck, place=p))
            p.verify()
        assert [k for k, _, _ in p.seen][:len(turns)] == turns


# ------------------------------------------------------------------------- device outputs capi never lets a caller place
@pytest.mark.parametrize("entry", ac.C_EDGES)
@stops_at_a_hip_error
def test_the_edges_of_the_c_abi_at_every_offset(ck, table, entry):
    """ck_board_edges, ck_goban_canny and ck_canny write `edges` (ck_canny `map_out` too) where the caller says; capi always
    says a fresh block, a C caller may say any byte.  The NMS kernel stores `edges` a dword at a time where map and edges lie
    on one (flat tiles and ordinary ones: the frames of the flat-tile rows have both); through ctypes, `edges` at every
    offset, `map_out` at the next one, against tests/filter_ref.py, the bands untouched."""
    import ctypes as C
    from camkifu_amd import capi
    from tests import filter_ref as fr
    L = capi.lib()
    frames = table["board_edges flat tiles"].args[0]
    table["board_edges flat tiles"].reaches()
    n, h, w, _ = frames.shape
    if entry == "ck_board_edges":
        want = [r["edges"] for r in table["board_edges flat tiles"].expect()]
    elif entry == "ck_goban_canny":
        want = [r["edges"] for r in table["goban_canny flat tiles"].expect()]
    else:
        refs = sc.expected("align canny flat tiles", lambda: [fr.canny(f, 25, 75) for f in frames])
        want, want_map = [r["edges"] for r in refs], [r["map"] for r in refs]
    assert any(e.any() for e in want) and not all(e.all() for e in want)
    src = np.ascontiguousarray(frames)
    offsets = ac.OFFSETS[1]
    for j, offset in enumerate(offsets):
        edges = ac.place(np.full((n, h, w), 0x33, np.uint8), offset)
        ck._order_behind_torch(edges.device)
        args = (ck._h, src.ctypes.data_as(C.c_void_p), n, h, w, capi.CK_HOST)
        if entry == "ck_board_edges":
            rc = L.ck_board_edges(*args, C.c_void_p(edges.data_ptr()), capi.CK_DEVICE)
        elif entry == "ck_goban_canny":
            otsu = np.zeros(n, np.float64)
            rc = L.ck_goban_canny(*args, C.c_void_p(edges.data_ptr()), capi.CK_DEVICE, otsu.ctypes.data_as(C.c_void_p))
        else:
            m = ac.place(np.full((n, h, w), 0x33, np.uint8), offsets[(j + 1) % len(offsets)])
            ck._order_behind_torch(m.device)
            rc = L.ck_canny(*args, 25, 75, C.c_void_p(edges.data_ptr()), C.c_void_p(m.data_ptr()), capi.CK_DEVICE)
        ck._chk(rc)
        ac.untouched(edges)
        got = edges.cpu().numpy()
        for f in range(n):
            assert np.array_equal(got[f], want[f]), "%s, edges at offset %d, frame %d: %d pixels differ" % (entry, offset, f, int((got[f] != want[f]).sum()))
        if entry == "ck_goban_canny":
            assert [float(v) for v in otsu] == [r["otsu"] for r in table["goban_canny flat tiles"].expect()]
        if entry == "ck_canny":
            ac.untouched(m)
            assert all(np.array_equal(m.cpu().numpy()[f], want_map[f]) for f in range(n)), (entry, offset)
