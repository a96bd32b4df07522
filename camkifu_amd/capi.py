"""ctypes binding of libck_hip.so -- the C-ABI declared in include/camkifu_amd.h.

This is the ONLY compute backend of the package: there is no CPU fallback.  If the shared
library has not been built, or no HIP device is present, the calls raise.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CK_HIP_LIB: developer override used to A/B kernel variants (tools/ab_variant.sh); never set in production
SO_PATH = os.environ.get("CK_HIP_LIB") or os.path.join(_HERE, "libck_hip.so")
CSRC = os.path.join(_HERE, "csrc")

CK_OK, CK_ERR_ARG, CK_ERR_HIP, CK_ERR_CAPACITY, CK_ERR_STATE, CK_ERR_DATA = 0, 1, 2, 3, 4, 5
CK_HOST, CK_DEVICE = 0, 1
CK_JPEG_GREY, CK_JPEG_444, CK_JPEG_422, CK_JPEG_420 = 0, 1, 2, 3
CK_JPEG_ENTROPY_HOST, CK_JPEG_ENTROPY_DEVICE = 0, 1
CK_JPEG_TABLES_STANDARD, CK_JPEG_TABLES_OPTIMISED = 0, 1
CK_JPEG_ENTROPY_DEVICE_SPANS = 2
CK_PNG_MATCH_NONE, CK_PNG_MATCH_RUNS = 0, 1
CK_PNG_INFLATE_HOST, CK_PNG_INFLATE_DEVICE = 0, 1
CK_CNN_FP32, CK_CNN_BF16, CK_CNN_F16X2, CK_CNN_F16Q8 = 0, 1, 2, 3
CK_CNN_DEFAULT = CK_CNN_F16X2            # what a new context computes in
CK_BOARD_LINES, CK_BOARD_NO_CONTOUR, CK_BOARD_TOO_SMALL = 0, 1, 2
CK_OV_SEGMENT, CK_OV_CIRCLE, CK_OV_DISC, CK_OV_RECT, CK_OV_TEXT = 1, 2, 3, 4, 5

ZONE_LINES = 32        # CK_ZONE_LINES

WEIGHT_ORDER = ("c1w", "c1b", "c2w", "c2b", "c3w", "c3b", "c4w", "c4b", "d1w", "d1b", "d2w", "d2b")
WEIGHT_SHAPES = dict(c1w=(5, 5, 3, 32), c1b=(32,), c2w=(5, 5, 32, 32), c2b=(32,),
                     c3w=(3, 3, 32, 90), c3b=(90,), c4w=(3, 3, 90, 90), c4b=(90,),
                     d1w=(3240, 160), d1b=(160,), d2w=(160, 81), d2b=(81,))


class BoardResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_contours", C.c_int32), ("n_lines", C.c_int32),
                ("reserved", C.c_int32), ("biggest_area", C.c_double)]


BOARD_DTYPE = np.dtype([("status", "<i4"), ("n_contours", "<i4"), ("n_lines", "<i4"), ("reserved", "<i4"),
                        ("biggest_area", "<f8")])          # ck_board_result, 24 bytes


REC_LMAX = 64                                               # CK_REC_LMAX
REC_LINES_CUT, REC_FAILED = 1, 2                            # CK_REC_*
REC_DTYPE = np.dtype([("status", "<i4"), ("n_contours", "<i4"), ("n_lines", "<i4"), ("flags", "<i4"),
                      ("biggest_area", "<f8"), ("lines", "<f4", (REC_LMAX, 2)),
                      ("region_conf", "<f8", (10, 10)), ("region_label", "u1", (10, 10)), ("pad", "u1", (4,))])   # ck_frame_record
REC_BYTES = REC_DTYPE.itemsize
if REC_BYTES != 1440:
    raise ImportError("REC_DTYPE is %d bytes, ck_frame_record is 1440" % REC_BYTES)


class CkError(RuntimeError):
    """`code`: the CK_ERR_* status of the call that failed (None where Python refused before calling); `bad_frame`: for a
    JPEG batch the decoder refused, the index of the stream it is about (else None)"""
    code = None
    bad_frame = None


class JpegInfo(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("sampling", C.c_int32), ("restart_interval", C.c_int32),
                ("blocks", C.c_int32)]                     # ck_jpeg_info


class PngInfo(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("color_type", C.c_int32), ("bit_depth", C.c_int32),
                ("palette_entries", C.c_int32), ("reserved", C.c_int32), ("rowbytes", C.c_longlong)]      # ck_png_info


def build(force=False):
    """Compile every HIP source for gfx950 into camkifu_amd/libck_hip.so (in-tree)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean", "-s"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    return SO_PATH


HEADER = os.path.join(_HERE, os.pardir, "include", "camkifu_amd.h")       # (where csrc/Makefile needs it too)
_SCALARS = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong,
            "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
_RETURNS = {"int": C.c_int, "void": None, "double": C.c_double, "const char*": C.c_char_p, "void*": C.c_void_p}


def _signatures(header=HEADER):
    """name -> (restype, argtypes) of every prototype the header declares: the one copy of the ABI on the Python side.
    A pointer or array parameter is c_void_p, a scalar maps by its C type; a type outside the tables is an error here,
    never a call with ctypes' defaults."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(header).read(), flags=re.S)
    sigs = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+[\s*]+)(ck_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        argtypes = []
        for prm in ([] if params.strip() in ("", "void") else params.split(",")):
            ctype = " ".join(w for w in prm.split()[:-1] if w != "const")
            if "*" not in prm and "[" not in prm and ctype not in _SCALARS:
                raise CkError("%s: no ctypes type for the parameter '%s'" % (name, prm.strip()))
            argtypes.append(C.c_void_p if "*" in prm or "[" in prm else _SCALARS[ctype])
        ret = " ".join(ret.replace("*", " * ").split()).replace(" *", "*")
        if ret not in _RETURNS:
            raise CkError("%s: no ctypes type for the return type '%s'" % (name, ret))
        sigs[name] = (_RETURNS[ret], argtypes)
    return sigs


_SIGNATURES = _signatures()
EXPORTS = sorted(_SIGNATURES)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise CkError("libck_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                          "camkifu_amd has no CPU fallback")
        # PyTorch-ROCm wheels bundle their own HIP runtime; two HIP runtimes in one process
        # cannot both own the GPU.  Importing torch first makes the loader resolve
        # libck_hip.so's libamdhip64.so.7 dependency to the copy torch already mapped, so
        # torch tensors and this library share one runtime (and one device context).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(SO_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def pyr_shape(h, w, levels):
    """(h, w) of the frames after `levels` applications of pyrDown: each side becomes (side + 1) // 2.  CkError, as from the
    library, for levels < 0 and for a level that would read an image with a side below 2."""
    h, w, levels = int(h), int(w), int(levels)
    if levels < 0:
        raise CkError("pyramid levels %d: negative" % levels)
    for l in range(levels):
        if h < 2 or w < 2:
            raise CkError("pyramid level %d would take a %dx%d image: sides below 2" % (l + 1, w, h))
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def _in(a, dtype=np.uint8):
    """-> (pointer, space, keepalive) for a numpy array or a torch tensor.  A DEVICE tensor must go through Context._in /
    Context._out instead (they order the context's stream behind torch's): this function refuses it."""
    if _is_torch(a):
        if a.is_cuda:
            raise CkError("a device tensor is handed to the library through Context._in / Context._out (stream-ordered hand-over)")
        a = a.numpy()
    a = np.ascontiguousarray(a, dtype)
    return a.ctypes.data_as(C.c_void_p), CK_HOST, a


def _check_array(a, shape, dtypes, what, writeable=False):
    """a numpy array or torch tensor the library reads or writes in place: shape (None: any), element type, contiguity (and
    for an array it writes, that numpy lets it) -- else CkError.  The library cannot know how much memory lies behind its pointers:
    sizes and element types are held on this side."""
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    if _is_torch(a):                 # (np.uint8.__name__ is the dtype's name too, and np.dtype.name takes microseconds)
        ok = a.is_contiguous() and str(a.dtype).replace("torch.", "") in [getattr(d, "__name__", None) or np.dtype(d).name for d in dtypes]
    elif isinstance(a, np.ndarray):
        ok = a.flags.c_contiguous and a.dtype in dtypes and (a.flags.writeable or not writeable)
    else:
        raise CkError("%s: a numpy array or a torch tensor is needed, got %s" % (what, type(a).__name__))
    if not ok or (shape is not None and tuple(a.shape) != tuple(shape)):
        raise CkError("%s: a contiguous%s %s array%s is needed, got %s %r" % (
            what, " writeable" if writeable else "", "/".join(np.dtype(d).name for d in dtypes),
            "" if shape is None else " of shape %r" % (tuple(shape),), str(a.dtype).replace("torch.", ""), tuple(a.shape)))


def _batch_of(a, tail, what):
    """n of `a`, n images of shape `tail` or one without the batch axis: the library reads n of exactly that size"""
    shp = tuple(a.shape)
    if shp[-len(tail):] != tail or len(shp) - len(tail) not in (0, 1):
        raise CkError("%s: shape (n,) + %r or %r is needed, got %r" % (what, tail, tail, shp))
    return 1 if len(shp) == len(tail) else shp[0]


class Context:
    """One ck_ctx: a HIP stream plus scratch buffers.  One per finder instance / thread."""

    def __init__(self, device=0, priority=0):
        """priority: HIP stream priority of the context's stream -- 0 normal, 1 highest, -1 lowest"""
        self._h = C.c_void_p()
        rc = lib().ck_ctx_create_prio(int(device), int(priority), C.byref(self._h))
        if rc != 0:
            raise CkError("ck_ctx_create failed: " + (lib().ck_last_error(None) or b"").decode())
        self.device = device
        self._mog2_shape = {}                    # handle -> (h, w) of the models this context created

    def close(self):
        """free the context.  A context another thread is still inside (for more than 5 s) is NOT freed and keeps its
        handle: CkError says so, and a later close() -- or the finaliser -- tries again (the handle used to be
        dropped regardless, the stream and all scratch HBM leaked with no way to retry)."""
        if self._h:
            if lib().ck_ctx_destroy2(self._h) != 0:
                raise CkError("the context is still inside a call on another thread: not freed, close() it again later")
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            err = CkError("libck_hip error %d: %s" % (rc, (lib().ck_last_error(self._h) or b"").decode()))
            err.code = rc
            raise err

    # ---- timing -------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._chk(lib().ck_timing_enable(self._h, int(on)))

    def timing_reset(self):
        self._chk(lib().ck_timing_reset(self._h))

    def timing_get(self, name):
        ms, cnt = C.c_double(0), C.c_int(0)
        self._chk(lib().ck_timing_get(self._h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def scratch_fill(self, byte):
        """a testing aid (ck_debug_scratch_fill): every byte of the context's scratch memory becomes `byte`, which must
        change no later result -> (bytes filled, buffers filled)"""
        nbytes, nbufs = C.c_longlong(0), C.c_int(0)
        self._chk(lib().ck_debug_scratch_fill(self._h, int(byte), C.byref(nbytes), C.byref(nbufs)))
        self._png_frames = 0                     # (the token counters went with the scratch: png_run_stats() is [] again)
        return int(nbytes.value), int(nbufs.value)

    # ---- helpers ---------------------------------------------------------------------------
    @staticmethod
    def _shape(img, cn):
        shp = tuple(img.shape)
        if len(shp) == 2 + (cn > 1):
            shp = (1,) + shp
        if len(shp) != 3 + (cn > 1) or (cn > 1 and shp[3] != cn):
            raise CkError("images of shape (n, h, w%s) or one without n are needed, got %r" % (", %d" % cn if cn > 1 else "", tuple(img.shape)))
        return shp[0], shp[1], shp[2]

    # Hand-over of DEVICE memory (torch tensors) -- the ONE place where it happens.  The library launches on the context's
    # own HIP stream; torch queues its kernels on the calling thread's current stream and reuses a freed block at once for
    # the next allocation on that stream, from any thread.  So before a pointer crosses the C-ABI the context's stream is
    # ordered behind torch's current stream (ck_stream_wait: an event recorded there, waited for here -- no host wait):
    # an input's producer has run, and so has the last kernel torch queued on a recycled output block (round 4: a memory
    # fault in a gather whose index tensor had been recycled into an output buffer).  Results need nothing in the other
    # direction: every entry point returns with its work complete.
    def _order_behind_torch(self, device):
        import torch
        self._chk(lib().ck_stream_wait(self._h, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))

    def _in(self, a, dtype=np.uint8, shape=None, what="array"):
        """an array the library reads -> (pointer, space, keepalive).  Host memory is converted to a C-contiguous array of
        `dtype` (a copy where it has to be); a device tensor is taken as it lies, so it must be contiguous and of exactly
        `dtype` (or one of a tuple of them, host memory being converted to the first).  `shape`: what the library will read,
        where the call does not tell it -- compared in both memory spaces."""
        if _is_torch(a) and a.is_cuda:
            _check_array(a, shape, dtype, what)
            self._order_behind_torch(a.device)
            return C.c_void_p(a.data_ptr()), CK_DEVICE, a
        p, sp, a = _in(a, dtype[0] if isinstance(dtype, tuple) else dtype)
        if shape is not None and a.shape != tuple(shape):
            raise CkError("%s: shape %r is needed, got %r" % (what, tuple(shape), a.shape))
        return p, sp, a

    def _out(self, like, shape, dtype, out=None, to_device=None):
        """the array the library writes -> (array, pointer, space): the caller's `out`, which is never copied (so it must
        be contiguous, writeable and of exactly this shape and dtype: the pointer handed over is its own), or else a fresh
        one on `to_device`, or else in the memory space of `like`"""
        if out is not None:
            if _is_torch(out) and out.is_cuda:
                return (out,) + self._in(out, dtype, shape, "out")[:2]
            _check_array(out, shape, dtype, "out", writeable=True)
            mem = out.numpy() if _is_torch(out) else out                # (a host tensor's array shares its memory)
            return out, mem.ctypes.data_as(C.c_void_p), CK_HOST
        if to_device is not None:
            return self._out_on(to_device, shape, dtype)
        if _is_torch(like) and like.is_cuda:
            return self._out_on(like.device, shape, dtype)
        a = np.empty(shape, dtype)
        return a, a.ctypes.data_as(C.c_void_p), CK_HOST

    def _out_on(self, device, shape, dtype):
        """a fresh device tensor the library may write: allocated, THEN the context's stream ordered behind torch's"""
        import torch
        t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=device)
        self._order_behind_torch(t.device)
        return t, C.c_void_p(t.data_ptr()), CK_DEVICE

    # ---- K1 ---------------------------------------------------------------------------------
    def median15(self, bgr):
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        out, op, osp = self._out(bgr, tuple(bgr.shape), np.uint8)
        self._chk(lib().ck_median15(self._h, p, n, h, w, sp, op, osp))
        return out

    def median(self, bgr, ksize):
        """cv2.medianBlur(bgr, ksize) for odd ksize in 3..17 (same matrix-core kernel, other window)"""
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        out, op, osp = self._out(bgr, tuple(bgr.shape), np.uint8)
        self._chk(lib().ck_median(self._h, p, n, h, w, int(ksize), sp, op, osp))
        return out

    def goban_canny(self, bgr, want_otsu=False):
        """SfContours.get_canny (stone/sf_contours.py:332-340): medianBlur 13 then 7, Otsu level of the grey image,
        Canny(median, otsu / 2, otsu) -> edges (and the Otsu levels)"""
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        edges, ep, osp = self._out(bgr, tuple(bgr.shape[:-1]), np.uint8)
        otsu = np.zeros(n, np.float64)
        self._chk(lib().ck_goban_canny(self._h, p, n, h, w, sp, ep, osp, otsu.ctypes.data_as(C.c_void_p)))
        return (edges, otsu) if want_otsu else edges

    # ---- K2 ---------------------------------------------------------------------------------
    def canny(self, img3, low=25, high=75, want_map=False):
        n, h, w = self._shape(img3, 3)
        p, sp, keep = self._in(img3)
        oshape = tuple(img3.shape[:-1])
        edges, ep, osp = self._out(img3, oshape, np.uint8)
        m, mp = None, None
        if want_map:
            m, mp, _ = self._out(img3, oshape, np.uint8)
        self._chk(lib().ck_canny(self._h, p, n, h, w, sp, int(low), int(high), ep, mp, osp))
        return (edges, m) if want_map else edges

    def board_edges(self, bgr):
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        edges, ep, osp = self._out(bgr, tuple(bgr.shape[:-1]), np.uint8)
        self._chk(lib().ck_board_edges(self._h, p, n, h, w, sp, ep, osp))
        return edges

    # ---- K3..K6 -------------------------------------------------------------------------------
    def _lines_out(self, n, cap, lines, res):
        out = []
        for f in range(n):
            k = min(res[f].n_lines, cap)
            out.append(dict(status=res[f].status, n_contours=res[f].n_contours, n_lines=res[f].n_lines,
                            biggest_area=res[f].biggest_area, lines=lines[f, :k].copy()))
        return out

    def board_lines(self, edges, hough_thresh=-1, cap=1024, want_ghost=False):
        n, h, w = self._shape(edges, 1)
        p, sp, keep = self._in(edges)
        lines = np.zeros((n, cap, 2), np.float32)
        res = (BoardResult * n)()
        ghost, gp, gsp = (None, None, CK_HOST)
        if want_ghost:
            ghost, gp, gsp = self._out(edges, tuple(edges.shape), np.uint8)
        self._chk(lib().ck_board_lines(self._h, p, n, h, w, sp, int(hough_thresh),
                                       lines.ctypes.data_as(C.c_void_p), cap, res, gp, gsp))
        out = self._lines_out(n, cap, lines, res)
        return (out, ghost) if want_ghost else out

    def board_detect(self, bgr, hough_thresh=-1, cap=1024, raw=False):
        """raw=True: (structured array of BOARD_DTYPE, lines (n, cap, 2)) without per-frame python objects"""
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        lines = np.zeros((n, cap, 2), np.float32)
        res = np.zeros(n, BOARD_DTYPE)
        self._chk(lib().ck_board_detect(self._h, p, n, h, w, sp, int(hough_thresh),
                                        lines.ctypes.data_as(C.c_void_p), cap, res.ctypes.data_as(C.c_void_p)))
        if raw:
            return res, lines
        return [dict(status=int(r["status"]), n_contours=int(r["n_contours"]), n_lines=int(r["n_lines"]),
                     biggest_area=float(r["biggest_area"]), lines=lines[f, :min(int(r["n_lines"]), cap)].copy())
                for f, r in enumerate(res)]

    # ---- per-frame result records, written in place (host memory or HBM) -------------------------------------------
    def wait_stream(self, stream):
        """everything queued on `stream` (a torch.cuda.Stream) up to now runs before anything this context launches from now
        on -- for a tensor another thread produced on a stream that is not this thread's current one (pipeline._take)"""
        self._chk(lib().ck_stream_wait(self._h, C.c_void_p(stream.cuda_stream)))

    def _rec(self, rec, n):
        """-> (pointer, space, keepalive) of n records: a C-contiguous numpy array of REC_DTYPE, or a contiguous torch uint8
        tensor (n, REC_BYTES) in HBM"""
        if _is_torch(rec):
            if tuple(rec.shape) != (n, REC_BYTES) or not rec.is_contiguous() or "uint8" not in str(rec.dtype):
                raise ValueError("records: expected a contiguous uint8 tensor of shape (%d, %d), got %r" % (n, REC_BYTES, tuple(rec.shape)))
            if rec.is_cuda:
                return self._in(rec)
            rec = rec.numpy().view(REC_DTYPE).reshape(n)
        if rec.dtype != REC_DTYPE or rec.shape != (n,) or not rec.flags.c_contiguous or not rec.flags.writeable:
            raise ValueError("records: expected a writeable C-contiguous array of %d REC_DTYPE rows" % n)
        return rec.ctypes.data_as(C.c_void_p), CK_HOST, rec

    def board_detect_records(self, bgr, rec, hough_thresh=-1):
        """K1..K6 of the frames -> the board half of their records, in place (ck_board_detect_records)"""
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        rp, rsp, keep2 = self._rec(rec, n)
        self._chk(lib().ck_board_detect_records(self._h, p, n, h, w, sp, int(hough_thresh), rp, rsp))
        return rec

    def _goban(self, goban):
        """n goban images (n, 380, 380, 3), or one (380, 380, 3), whose size the library takes for granted -> (n,) + _in()"""
        n = _batch_of(goban, (380, 380, 3), "goban")
        return (n,) + self._in(goban, what="goban")

    def cnn_regions_records(self, goban, rec):
        """K10..K12 of the goban images -> the stones half of their records, in place (ck_cnn_regions_records)"""
        n, p, sp, keep = self._goban(goban)
        rp, rsp, keep2 = self._rec(rec, n)
        self._chk(lib().ck_cnn_regions_records(self._h, p, n, sp, rp, rsp))
        return rec

    # ---- frame source ------------------------------------------------------------------------
    def i420_to_bgr(self, i420, h, w, to_device=None, out=None, levels=0):
        """planar YUV 4:2:0 frames (n, h*w*3/2) or one flat frame -> BGR (n, h, w, 3) / (h, w, 3).
        `to_device`: a torch device to leave the BGR frames in HBM even when the I420 bytes come from host memory (the
        fast-file path uploads 1.5 B/px and converts on the GPU); `out`: a preallocated BGR tensor / array to fill.
        `levels` > 0: the frames come out pyrDown-ed that many times, of shape pyr_shape(h, w, levels) -- bit for bit
        pyr_down(i420_to_bgr(..), levels), but the full-size BGR frames are never written (ck_i420_to_bgr_pyr)."""
        h, w, levels = int(h), int(w), int(levels)
        single = len(i420.shape) == 1
        n = _batch_of(i420, (h * w * 3 // 2,), "i420")
        if levels and ((h | w) & 1):
            raise CkError("I420 needs even dimensions, got %dx%d" % (w, h))
        oh, ow = pyr_shape(h, w, levels)
        p, sp, keep = self._in(i420, what="i420")
        out, op, osp = self._out(i420, (oh, ow, 3) if single else (n, oh, ow, 3), np.uint8, out, to_device if sp == CK_HOST else None)
        if levels:
            self._chk(lib().ck_i420_to_bgr_pyr(self._h, p, n, h, w, levels, sp, op, osp))
        else:
            self._chk(lib().ck_i420_to_bgr(self._h, p, n, h, w, sp, op, osp))
        return out

    def jpeg_decode(self, streams, to_device=None, out=None):
        """baseline JPEG streams (a list of bytes-like objects or uint8 arrays in host memory, all of the first one's size
        and sampling) -> BGR frames (n, h, w, 3), bit for bit what cv2.imread gives.  Huffman decoding runs on the host (the
        frames of a batch in parallel), everything after it in one kernel.  `to_device`: a torch device to leave the frames
        in HBM; `out`: a preallocated (n, h, w, 3) array / tensor to fill.  CkError with code CK_ERR_DATA and a message
        that names the frame and the cause for a stream the decoder refuses or that is damaged."""
        ptrs, lens, keep = _jpeg_streams(streams)
        n = len(keep)
        rc, info, why = _jpeg_probe(keep[0])          # (the size of the output comes from the first stream's headers)
        if rc != 0:
            err = CkError("libck_hip error %d: frame 0: %s" % (rc, why))
            err.code, err.bad_frame = rc, 0
            raise err
        out, op, osp = self._out(None, (n, info["h"], info["w"], 3), np.uint8, out, to_device)
        rc = lib().ck_jpeg_decode(self._h, ptrs, lens, n, op, osp)
        if rc == CK_ERR_DATA:
            bad = C.c_int32(-1)
            err = CkError("libck_hip error %d: %s" % (rc, (lib().ck_last_error(self._h) or b"").decode()))
            err.code = rc
            if lib().ck_jpeg_bad_frame(self._h, C.byref(bad)) == 0 and bad.value >= 0:
                err.bad_frame = bad.value
            raise err
        self._chk(rc)
        return out

    def jpeg_set_entropy(self, mode):
        """where jpeg_decode runs the Huffman stage from now on: "host" (the default: the library's worker threads) or
        "device" (one GPU lane per restart interval; the compressed bytes go up instead of the coefficients), or
        "device-spans" (the same upload, decoded in parallel inside a restart interval as well: a lane per span of
        jpeg_set_span_bytes bytes)"""
        modes = {"host": CK_JPEG_ENTROPY_HOST, "device": CK_JPEG_ENTROPY_DEVICE, "device-spans": CK_JPEG_ENTROPY_DEVICE_SPANS}
        if mode not in modes:
            raise CkError("jpeg entropy mode: 'host' or 'device' is needed (or 'device-spans'), got %r" % (mode,))
        self._chk(lib().ck_jpeg_set_entropy(self._h, modes[mode]))

    def jpeg_set_span_bytes(self, nbytes):
        """the span size of the "device-spans" mode, 8 .. 4096 bytes (jpeg_span_bytes() gives the default)"""
        self._chk(lib().ck_jpeg_set_span_bytes(self._h, int(nbytes)))

    def jpeg_span_stats(self):
        """what the last jpeg_decode / jpeg_coefficients_device of this context did in "device-spans" mode -> dict(spans,
        unresolved, suspect_strands, one_lane_frames)"""
        st = (C.c_longlong * 4)()
        self._chk(lib().ck_jpeg_span_stats(self._h, st))
        return dict(zip(JPEG_SPAN_STATS, (int(v) for v in st)))

    def jpeg_uploaded_bytes(self):
        """the bytes the last jpeg_decode or jpeg_coefficients_device of this context copied from host to device"""
        b = C.c_longlong(0)
        self._chk(lib().ck_jpeg_uploaded_bytes(self._h, C.byref(b)))
        return b.value

    def jpeg_coefficients_device(self, streams, to_device=None):
        """jpeg_coefficients with the Huffman stage on the GPU: streams of one geometry in host memory -> (info of the
        first, coef (n, blocks * 64) int16, quant (n, 3, 64)) as numpy arrays (quant uint16), or with `to_device` as torch
        tensors in HBM (quant int16: the bits count).  CkError (CK_ERR_DATA) names the frame that failed; its index is
        the error's `bad_frame`."""
        ptrs, lens, keep = _jpeg_streams(streams)
        n = len(keep)
        info = jpeg_probe(keep[0])
        geom = JpegInfo(info["h"], info["w"], info["sampling"], info["restart_interval"], info["blocks"])
        coef, cp, sp = self._out(None, (n, info["blocks"] * 64), np.int16, None, to_device)
        quant, qp, _ = self._out(None, (n, 3, 64), np.uint16 if to_device is None else np.int16, None, to_device)
        bad = C.c_int32(-1)
        rc = lib().ck_jpeg_coefficients_device(self._h, ptrs, lens, n, C.byref(geom), cp, qp, sp, C.byref(bad))
        if rc != 0:
            err = CkError("libck_hip error %d: %s" % (rc, (lib().ck_last_error(self._h) or b"").decode()))
            err.code = rc
            if bad.value >= 0:
                err.bad_frame = bad.value
            raise err
        return info, coef, quant

    def jpeg_reconstruct(self, coef, quant, h, w, sampling, out=None):
        """the GPU half alone: coefficients (n, blocks * 64) int16 and quant tables (n, 3, 64) uint16 as jpeg_coefficients
        gives them (numpy arrays, or torch tensors in HBM) -> BGR (n, h, w, 3) in the memory space of the input"""
        n, h, w, sampling = int(coef.shape[0]), int(h), int(w), int(sampling)
        _check_array(coef, (n, jpeg_blocks(h, w, sampling) * 64), np.int16, "coef")
        _check_array(quant, (n, 3, 64), (np.uint16, np.int16), "quant")          # (torch below 2.3 has no uint16: the bits count)
        cp, sp, keep = self._in(coef, np.int16)
        qp, qsp, keep2 = self._in(quant, (np.uint16, np.int16))
        if sp != qsp:
            raise CkError("coef and quant must lie in the same memory space")
        out, op, osp = self._out(coef, (n, h, w, 3), np.uint8, out)
        self._chk(lib().ck_jpeg_reconstruct(self._h, cp, qp, n, h, w, sampling, sp, op, osp))
        return out

    def jpeg_forward(self, frames, quant, sampling=CK_JPEG_420, out=None):
        """the GPU half of the encoder alone: BGR frames (n, h, w, 3) or one frame (h, w, 3), numpy or a torch tensor in HBM,
        and one set of quant tables (3, 64) as jpeg_quant gives them -> coefficients (n, blocks * 64) int16 in the memory
        space of the input, in the layout jpeg_coefficients gives and jpeg_reconstruct takes"""
        _check_frames(frames)
        n, h, w = self._shape(frames, 3)
        sampling = int(sampling)
        quant = _quant_tables(quant)
        p, sp, keep = self._in(frames)
        out, op, osp = self._out(frames, (n, jpeg_blocks(h, w, sampling) * 64), np.int16, out)
        self._chk(lib().ck_jpeg_forward(self._h, p, n, h, w, sp, quant.ctypes.data_as(C.c_void_p), sampling, op, osp))
        return out

    def jpeg_encode(self, frames, quality=90, sampling=CK_JPEG_420, restart_interval=0, optimize=False):
        """BGR frames (n, h, w, 3) or one frame (h, w, 3), numpy or a torch tensor in HBM -> a list of n `bytes`: baseline
        JPEG streams, byte for byte what PIL.Image.save(.., "JPEG", quality=quality, subsampling=..) writes.  The forward
        kernel runs on the GPU; the Huffman coder on the host (the frames of a batch in parallel), or, after
        jpeg_set_encode_entropy("device"), on the GPU as well: then the coefficients stay in HBM and only the streams come
        down.  The bytes are the same in both modes.  restart_interval in MCUs, 0: none.  optimize=True: Huffman tables
        fitted to each frame for this call, the bytes of PIL's optimize=True -- the same pixels in a smaller stream;
        False: what jpeg_set_encode_tables has set (the standard tables in a new context)."""
        if optimize and self._jpeg_tables != "optimised":
            self.jpeg_set_encode_tables("optimised")
            try:
                return self.jpeg_encode(frames, quality, sampling, restart_interval)
            finally:
                self.jpeg_set_encode_tables("standard")
        _check_frames(frames)
        n, h, w = self._shape(frames, 3)
        sampling = int(sampling)
        stride = jpeg_encode_bound(h, w, sampling)
        p, sp, keep = self._in(frames)
        out = np.empty(n * stride, np.uint8)             # (pages the streams do not reach are never touched)
        lens = (C.c_size_t * n)()
        self._chk(lib().ck_jpeg_encode(self._h, p, n, h, w, sp, int(quality), sampling, int(restart_interval),
                                       out.ctypes.data_as(C.c_void_p), stride, lens))
        return [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)]

    def jpeg_set_encode_entropy(self, mode):
        """where jpeg_encode runs the Huffman stage from now on: "host" (the default: the library's worker threads) or
        "device" (every block sizes its own code, prefix sums place the blocks and the stuffed bytes; only the streams
        come down)"""
        modes = {"host": CK_JPEG_ENTROPY_HOST, "device": CK_JPEG_ENTROPY_DEVICE}
        if mode not in modes:
            raise CkError("jpeg entropy mode: 'host' or 'device' is needed, got %r" % (mode,))
        self._chk(lib().ck_jpeg_set_encode_entropy(self._h, modes[mode]))

    _jpeg_tables = "standard"

    def jpeg_set_encode_tables(self, mode):
        """the Huffman tables jpeg_encode writes from now on, in either entropy mode: "standard" (the default: Annex K.3)
        or "optimised" (fitted to each frame, libjpeg's optimize_coding)"""
        modes = {"standard": CK_JPEG_TABLES_STANDARD, "optimised": CK_JPEG_TABLES_OPTIMISED}
        if mode not in modes:
            raise CkError("jpeg encode tables: 'standard' or 'optimised' is needed, got %r" % (mode,))
        self._chk(lib().ck_jpeg_set_encode_tables(self._h, modes[mode]))
        self._jpeg_tables = mode

    def jpeg_encode_histograms(self, n):
        """a test hook: the symbol counters the GPU kernels left in HBM in the last pass of this context's last optimised
        encode in the device mode -> (n, 4, 256) uint32, as jpeg_histogram gives them; n: the frames of that pass"""
        counts = np.zeros((int(n), 4, 256), np.uint32)
        self._chk(lib().ck_jpeg_encode_histograms(self._h, int(n), counts.ctypes.data_as(C.c_void_p)))
        return counts

    def jpeg_downloaded_bytes(self):
        """the bytes the last jpeg_encode or jpeg_entropy_encode_device of this context copied from device to host"""
        b = C.c_longlong(0)
        self._chk(lib().ck_jpeg_downloaded_bytes(self._h, C.byref(b)))
        return b.value

    def jpeg_entropy_encode_device(self, coef, quant, h, w, sampling, restart_interval=0, optimize=False):
        """jpeg_entropy_encode with the Huffman stage on the GPU: coefficients (n, blocks * 64) int16, a numpy array or a
        torch tensor in HBM, + one set of quant tables (3, 64) -> a list of n `bytes`, those of the host coder.  CkError
        (CK_ERR_ARG) for a coefficient the baseline Huffman tables cannot code, in the host coder's words.  optimize=True:
        tables fitted to each frame, counted and built on the GPU (ck_jpeg_entropy_encode_opt_device)."""
        h, w, sampling = int(h), int(w), int(sampling)
        n = int(coef.shape[0]) if len(coef.shape) == 2 else -1
        _check_array(coef, (n, jpeg_blocks(h, w, sampling) * 64), np.int16, "coef")
        quant = _quant_tables(quant)
        stride = jpeg_encode_bound(h, w, sampling)
        p, sp, keep = self._in(coef, np.int16)
        out = np.empty(max(1, n) * stride, np.uint8)
        lens = (C.c_size_t * max(1, n))()
        fn = lib().ck_jpeg_entropy_encode_opt_device if optimize else lib().ck_jpeg_entropy_encode_device
        self._chk(fn(self._h, p, sp, quant.ctypes.data_as(C.c_void_p), n, h, w, sampling,
                     int(restart_interval), out.ctypes.data_as(C.c_void_p), stride, lens))
        return [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)]

    _png_inflate = "host"

    def png_set_inflate(self, mode):
        """where png_decode inflates from now on: "host" (the default: the library's worker threads) or "device" (a wave per
        zlib stream on the GPU; only the compressed bytes go up).  Both accept and refuse the same files with the same
        message and give the same pixels; one stream keeps one wave busy, so the device mode is for batches."""
        modes = {"host": CK_PNG_INFLATE_HOST, "device": CK_PNG_INFLATE_DEVICE}
        if mode not in modes:
            raise CkError("png inflate: 'host' or 'device' is needed, got %r" % (mode,))
        self._chk(lib().ck_png_set_inflate(self._h, modes[mode]))
        self._png_inflate = mode

    def png_inflate_device(self, streams, cap=None):
        """the inflate kernel alone: zlib streams (bytes-like objects or uint8 arrays in host memory), one wave each in one
        launch -> a list with dict(data, total, cause, produced) for each: the first `cap` bytes (an int for all streams or
        one for each; None: 65536), the count of all bytes (0 for a refused stream), 0 or the cause of the refusal (the
        CK_INF_* of csrc/ck_png_inflate_stage.h, as png_inflate_staged(verdict=True) gives it) and the bytes inflated in
        front of what was refused.  data is None for a refused stream: it does not fail the call."""
        ptrs, lens, keep = _jpeg_streams(streams)
        n = len(keep)
        caps = [65536 if cap is None else int(cap)] * n if cap is None or isinstance(cap, (int, np.integer)) else [int(c) for c in cap]
        if len(caps) != n or min(caps) < 0:
            raise CkError("png_inflate_device: one cap >= 0 for each of the %d streams is needed" % n)
        stride = max(16, max(caps))
        out = np.empty(n * stride, np.uint8)
        total, cause, produced = (C.c_size_t * n)(), (C.c_int32 * n)(), (C.c_longlong * n)()
        self._chk(lib().ck_png_inflate_device(self._h, ptrs, lens, n, out.ctypes.data_as(C.c_void_p), (C.c_size_t * n)(*caps), stride,
                                              total, cause, produced))
        return [dict(data=None if cause[f] else out[f * stride:f * stride + min(caps[f], total[f])].tobytes(), total=int(total[f]),
                     cause=int(cause[f]), produced=int(produced[f])) for f in range(n)]

    def png_uploaded_bytes(self):
        """the bytes this context's last png_decode copied to the GPU, all passes: inflated rows in the host mode, zlib
        streams in the device mode, descriptors and palettes in both"""
        b = C.c_longlong(0)
        self._chk(lib().ck_png_uploaded_bytes(self._h, C.byref(b)))
        return b.value

    def png_inflate_stats(self):
        """the inflate kernel's counts for this context's last png_decode in device mode or png_inflate_device ->
        dict(streams, steps, tokens, bytes): window steps, literals and matches applied, bytes produced"""
        v = (C.c_longlong * 4)()
        self._chk(lib().ck_png_inflate_stats(self._h, v))
        return dict(zip(("streams", "steps", "tokens", "bytes"), (int(x) for x in v)))

    def png_decode(self, streams, to_device=None, out=None, inflate=None):
        """PNG files (a list of bytes-like objects or uint8 arrays in host memory, all of the first one's height and width,
        each of its own colour type, bit depth and palette) -> BGR frames (n, h, w, 3), what cv2.imread gives: alpha dropped,
        16-bit samples cut to their high byte.  The chunk walk and the inflate run on the host (the frames of a batch in
        parallel), the unfiltering and the expansion to BGR in one kernel.  `to_device`: a torch device to leave the frames
        in HBM; `out`: a preallocated (n, h, w, 3) array / tensor to fill.  inflate: "host" / "device" for this call, None
        takes what png_set_inflate has set (the host in a new context).  CkError with code CK_ERR_DATA and a message that
        names the frame and the cause for a file the reader refuses or that is damaged; its index is the error's `bad_frame`."""
        if inflate is not None and inflate != self._png_inflate:
            was = self._png_inflate
            self.png_set_inflate(inflate)
            try:
                return self.png_decode(streams, to_device, out)
            finally:
                self.png_set_inflate(was)
        ptrs, lens, keep = _jpeg_streams(streams)
        n = len(keep)
        info = PngInfo()
        rc = lib().ck_png_header(C.c_void_p(keep[0].ctypes.data), keep[0].size, C.byref(info))     # (the size of the output)
        if rc != 0:
            err = CkError("libck_hip error %d: frame 0: %s" % (rc, (lib().ck_last_error(None) or b"").decode()))
            err.code, err.bad_frame = rc, 0
            raise err
        out, op, osp = self._out(None, (n, info.h, info.w, 3), np.uint8, out, to_device)
        bad = C.c_int32(-1)
        rc = lib().ck_png_decode(self._h, ptrs, lens, n, op, osp, C.byref(bad))
        if rc != 0:
            err = CkError("libck_hip error %d: %s" % (rc, (lib().ck_last_error(self._h) or b"").decode()))
            err.code = rc
            if bad.value >= 0:
                err.bad_frame = bad.value
            raise err
        return out

    _png_matches = "none"

    def png_set_encode_matches(self, mode):
        """what png_encode makes of repeated bytes from now on: "none" (the default: literals only) or "runs" (inside a band
        every run of equal filtered bytes is one literal and matches of distance 1 behind it: what zlib's Z_RLE gains on flat
        images; the same pixels come back)"""
        modes = {"none": CK_PNG_MATCH_NONE, "runs": CK_PNG_MATCH_RUNS}
        if mode not in modes:
            raise CkError("png encode matches: 'none' or 'runs' is needed, got %r" % (mode,))
        self._chk(lib().ck_png_set_encode_matches(self._h, modes[mode]))
        self._png_matches = mode

    def png_run_stats(self):
        """the tokens of this context's last png_encode -> a list with dict(literals, matches) for each of its frames (the
        end-of-block symbols are not counted; matches is 0 in the literal-only mode), read from the histograms the count
        step left in HBM; [] where this context has encoded nothing yet or its last png_encode failed"""
        n = self._png_frames
        if n == 0:
            return []
        lit, mat = (C.c_longlong * n)(), (C.c_longlong * n)()
        self._chk(lib().ck_png_run_stats(self._h, n, lit, mat))
        return [dict(literals=int(lit[f]), matches=int(mat[f])) for f in range(n)]

    _png_frames = 0

    def png_encode(self, frames, filter=None, runs=None):
        """BGR frames (n, h, w, 3) or one frame (h, w, 3), numpy or a torch tensor in HBM -> a list of n `bytes`: 8-bit RGB
        PNG files with one IDAT chunk.  filter: None chooses per row the type with the least sum of absolute residuals
        (libpng's heuristic), 0 .. 4 forces None / Sub / Up / Avg / Paeth.  runs: True / False asks for the runs mode or the
        literal-only mode for this call, None takes what png_set_encode_matches has set (literals only in a new context).
        Filtering, the Huffman codes (one deflate block per band of png_tiles()["band_rows"] rows), the bit packing and the
        Adler-32 run on the GPU; only the zlib streams come down, the chunks and their CRCs are put around them on the host."""
        if runs is not None and ("runs" if runs else "none") != self._png_matches:
            was = self._png_matches
            self.png_set_encode_matches("runs" if runs else "none")
            try:
                return self.png_encode(frames, filter)
            finally:
                self.png_set_encode_matches(was)
        _check_frames(frames)
        n, h, w = self._shape(frames, 3)
        stride = png_encode_bound(h, w)
        p, sp, keep = self._in(frames)
        out = np.empty(n * stride, np.uint8)             # (pages the files do not reach are never touched)
        lens = (C.c_size_t * n)()
        self._png_frames = 0
        self._chk(lib().ck_png_encode(self._h, p, n, h, w, sp, _png_filter(filter), out.ctypes.data_as(C.c_void_p), stride, lens))
        self._png_frames = n
        return [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)]

    def overlay_draw(self, images, lists):
        """draw display lists (core.overlay.DisplayList) on uint8 images, in place, and return `images`: one list for one
        image (h, w) / (h, w, c), or a sequence of n lists for a batch (n, h, w) / (n, h, w, c), c in {1, 3}; a numpy
        array (C-contiguous, writeable) or a torch tensor in HBM.  One kernel launch for the whole batch
        (ck_overlay_draw); the rules of every primitive are in include/camkifu_amd.h."""
        from .core.overlay import DisplayList, pack
        single = isinstance(lists, DisplayList)
        lists = [lists] if single else list(lists)
        shp = tuple(images.shape)
        name = str(images.dtype).replace("torch.", "")
        lead = 0 if single else 1
        if name != "uint8" or len(shp) not in (lead + 2, lead + 3):
            raise CkError("images: a uint8 array of shape %s is needed, got %s %r" % (
                "(h, w) or (h, w, c)" if single else "(n, h, w) or (n, h, w, c)", name, shp))
        n = 1 if single else shp[0]
        h, w = shp[lead], shp[lead + 1]
        c = shp[lead + 2] if len(shp) == lead + 3 else 1
        if len(lists) != n:
            raise CkError("%d display lists for %d images" % (len(lists), n))
        if _is_torch(images):
            if not images.is_contiguous():
                raise CkError("images: a contiguous tensor is needed")
            if images.is_cuda:
                p, sp, keep = self._in(images)
            else:
                keep = images.numpy()                            # (shares the tensor's memory)
                p, sp = keep.ctypes.data_as(C.c_void_p), CK_HOST
        elif isinstance(images, np.ndarray) and images.flags.c_contiguous and images.flags.writeable:
            p, sp, keep = images.ctypes.data_as(C.c_void_p), CK_HOST, images
        else:
            raise CkError("images: a C-contiguous writeable numpy array or a torch tensor is needed (the drawing is in place)")
        prims, start, text = pack(lists)
        self._chk(lib().ck_overlay_draw(self._h, p, n, h, w, c, sp, prims.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                                        C.c_char_p(text), len(text)))
        return images

    def pyr_down(self, frames, levels=1, out=None):
        """cv2.pyrDown of BGR frames (n, h, w, 3) or one frame (h, w, 3), applied `levels` (>= 1) times -> frames of
        pyr_shape(h, w, levels) in the memory space of the input; `out`: a preallocated array / tensor to fill."""
        n, h, w = self._shape(frames, 3)
        levels = int(levels)
        if levels < 1:
            raise CkError("pyramid levels %d: at least 1" % levels)
        oh, ow = pyr_shape(h, w, levels)
        p, sp, keep = self._in(frames)
        out, op, osp = self._out(frames, (oh, ow, 3) if len(frames.shape) == 3 else (n, oh, ow, 3), np.uint8, out)
        self._chk(lib().ck_pyr_down(self._h, p, n, h, w, levels, sp, op, osp))
        return out

    # ---- K8 ---------------------------------------------------------------------------------
    def warp_perspective(self, bgr, M, dsize=380, out=None):
        """`out`: an (n, dsize, dsize, 3) uint8 array / tensor in the same memory space as `bgr` to write into"""
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        M = np.ascontiguousarray(M, np.float64).reshape(-1, 9)
        out, op, osp = self._out(bgr, (dsize, dsize, 3) if len(bgr.shape) == 3 else (n, dsize, dsize, 3), np.uint8, out)
        if osp != sp:
            raise CkError("out must live where the frames live")
        self._chk(lib().ck_warp_perspective(self._h, p, n, h, w, sp, M.ctypes.data_as(C.c_void_p), len(M),
                                            int(dsize), op, osp))
        return out

    # ---- K9 ---------------------------------------------------------------------------------
    def mog2_create(self, h=380, w=380):
        hd = C.c_int(-1)
        self._chk(lib().ck_mog2_create(self._h, h, w, C.byref(hd)))
        self._mog2_shape[hd.value] = (int(h), int(w))
        return hd.value

    def _mog2_hw(self, handle):
        """(h, w) of a model this context created: the size of what the library reads and writes for it.  Any other handle
        is refused in the library's own words, before a size is taken on trust"""
        st = self._mog2_shape.get(int(handle))
        if st is None:
            err = CkError("libck_hip error %d: bad mog2 handle %d" % (CK_ERR_ARG, int(handle)))
            err.code = CK_ERR_ARG
            raise err
        return st

    def mog2_apply(self, handle, img3, learning_rate):
        h, w = self._mog2_hw(handle)
        if _batch_of(img3, (h, w, 3), "img3") != 1:
            raise CkError("img3: one image of the model's %dx%d is needed, got %r" % (w, h, tuple(img3.shape)))
        p, sp, keep = self._in(img3, what="img3")
        fg, fp_, osp = self._out(img3, tuple(img3.shape[:-1]), np.uint8)
        self._chk(lib().ck_mog2_apply(self._h, int(handle), p, sp, learning_rate, fp_, osp))
        return fg

    def mog2_state(self, handle):
        """the model's mixture on the host: dict(weight (5, npx) f32, variance (5, npx) f32, mean (5, 3, npx) f32,
        nmodes (npx,) u8), npx = h * w; slots k >= nmodes[px] are unspecified"""
        st = self._mog2_hw(handle)
        npx = st[0] * st[1]
        out = dict(weight=np.empty((5, npx), np.float32), variance=np.empty((5, npx), np.float32),
                   mean=np.empty((5, 3, npx), np.float32), nmodes=np.empty(npx, np.uint8))
        self._chk(lib().ck_mog2_get_state(self._h, int(handle), *(out[k].ctypes.data_as(C.c_void_p)
                                                                  for k in ("weight", "variance", "mean", "nmodes"))))
        return out

    def mog2_destroy(self, handle):
        self._chk(lib().ck_mog2_destroy(self._h, int(handle)))
        self._mog2_shape.pop(int(handle), None)

    # ---- K10..K12 ----------------------------------------------------------------------------
    def cnn_set_weights(self, weights):
        """weights: dict name -> float32 array (numpy, or torch tensors all on cuda / all on cpu)."""
        ptrs, space, keep = self._weight_ptrs(weights, "weights")
        self._chk(lib().ck_cnn_set_weights(self._h, ptrs, space))

    def cnn_set_mode(self, mode):
        self._chk(lib().ck_cnn_set_mode(self._h, int(mode)))

    def cnn_predict(self, goban, want_y=True):
        n, p, sp, keep = self._goban(goban)
        y, yp = None, None
        if want_y:
            y, yp, _ = self._out(goban, (n, 100, 81), np.float32)
        labels, lp, osp = self._out(goban, (n, 19, 19), np.uint8)
        conf, cp, _ = self._out(goban, (n, 19, 19), np.float64)
        self._chk(lib().ck_cnn_predict(self._h, p, n, sp, yp, lp, cp, osp))
        return (y, labels, conf) if want_y else (labels, conf)

    def cnn_maps(self, goban):
        """the classifier's pooled filter maps as the context's mode computes them (host float32, channels-last):
        (pool2 (n, 100, 16, 16, 32), pool4 (n, 100, 6, 6, 90)) -- the outputs of the two MaxPooling2D layers of
        create_net (stone/nn_manager.py:280-292); n <= 128"""
        n, p, sp, keep = self._goban(goban)
        p2 = np.empty((n, 100, 16, 16, 32), np.float32)
        p4 = np.empty((n, 100, 6, 6, 90), np.float32)
        self._chk(lib().ck_cnn_maps(self._h, p, n, sp, p2.ctypes.data_as(C.c_void_p), p4.ctypes.data_as(C.c_void_p)))
        return p2, p4

    # ---- training of the classifier (k_cnn_train.hip) -----------------------------------------
    def _weight_ptrs(self, arrays, what):
        """12 float32 arrays under the WEIGHT_ORDER names -> (pointer table, memory space, keepalive).  Host arrays of another
        element type are cast; a device tensor has to be float32 (CkError)"""
        ptrs, keep, space = (C.c_void_p * 12)(), [], None
        for i, k in enumerate(WEIGHT_ORDER):
            a = arrays[k]
            if tuple(a.shape) != WEIGHT_SHAPES[k]:
                raise ValueError("%s %s: shape %r, expected %r" % (what, k, tuple(a.shape), WEIGHT_SHAPES[k]))
            p, sp, ka = self._in(a.contiguous() if _is_torch(a) else a, np.float32, what="%s %s" % (what, k))
            if space not in (None, sp):
                raise ValueError("%s must live in one memory space" % what)
            space, ptrs[i] = sp, p
            keep.append(ka)
        return ptrs, space, keep

    @staticmethod
    def _weight_outs():
        out = {k: np.empty(WEIGHT_SHAPES[k], np.float32) for k in WEIGHT_ORDER}
        return out, (C.c_void_p * 12)(*(out[k].ctypes.data_as(C.c_void_p) for k in WEIGHT_ORDER))

    def train_create(self, weights):
        """a trainer holding a copy of `weights` (dict of 12 float32 arrays, numpy or torch, host or device) -> handle"""
        ptrs, space, keep = self._weight_ptrs(weights, "weights")
        hd = C.c_int(-1)
        self._chk(lib().ck_train_create(self._h, ptrs, space, C.byref(hd)))
        return hd.value

    def train_destroy(self, handle):
        self._chk(lib().ck_train_destroy(self._h, int(handle)))

    def _train_batch(self, x, labels):
        """-> (pointer, space, n, h, w, c, labels pointer, keepalive); the library checks the shape and the labels"""
        shp = tuple(int(v) for v in x.shape) + (0,) * 4
        n, h, w, c = shp[:4] if len(x.shape) == 4 else (shp[0], 0, 0, 0)
        if _is_torch(labels):
            labels = labels.detach().cpu().numpy()
        labels = np.asarray(labels)
        if labels.ndim == 2:                         # one-hot rows
            labels = labels.argmax(1)
        if labels.shape != (n,):
            raise ValueError("labels %r for %d patches" % (labels.shape, n))
        lab = np.ascontiguousarray(np.where((labels < 0) | (labels > 255), 255, labels), np.uint8)      # out of range: the library says so
        if _is_torch(x):
            x = x.contiguous()
        p, sp, keep = self._in(x)
        return p, sp, n, h, w, c, lab.ctypes.data_as(C.c_void_p), (keep, lab)

    def train_step(self, handle, x, labels, lr=0.001, dropout=True, seed=0):
        """gradients of the batch and one Adam update -> the batch's mean loss (before the update).  x: uint8 (n, 40, 40, 3)
        raw BGR patches, host or device; labels: n class indices 0..80 (or one-hot rows)"""
        p, sp, n, h, w, c, lp, keep = self._train_batch(x, labels)
        loss = C.c_float(0)
        self._chk(lib().ck_train_step(self._h, int(handle), p, lp, n, h, w, c, sp, lr, int(bool(dropout)),
                                      int(seed) & 0xffffffffffffffff, C.byref(loss)))
        return float(loss.value)

    def train_grads(self, handle, x, labels, dropout=False, seed=0, step=-1):
        """the inspection call: (loss, dict of the 12 gradients, masks) with no update; masks = the three keep-masks
        (n, 16, 16, 32), (n, 6, 6, 90), (n, 160) as uint8 with dropout, else None.  step < 0: the trainer's own count"""
        p, sp, n, h, w, c, lp, keep = self._train_batch(x, labels)
        grads, gp = self._weight_outs()
        loss = C.c_float(0)
        masks, mp = None, [None] * 3
        if dropout:
            masks = [np.empty((n,) + s, np.uint8) for s in ((16, 16, 32), (6, 6, 90), (160,))]
            mp = [m.ctypes.data_as(C.c_void_p) for m in masks]
        self._chk(lib().ck_train_grads(self._h, int(handle), p, lp, n, h, w, c, sp, int(bool(dropout)),
                                       int(seed) & 0xffffffffffffffff, int(step), C.byref(loss), gp, *mp))
        return float(loss.value), grads, masks

    def train_apply(self, handle, grads, lr=0.001):
        """one Adam update from 12 given gradient arrays (host)"""
        host = {k: (grads[k].detach().cpu().numpy() if _is_torch(grads[k]) else grads[k]) for k in WEIGHT_ORDER}
        ptrs, space, keep = self._weight_ptrs(host, "gradients")
        self._chk(lib().ck_train_apply(self._h, int(handle), ptrs, lr))

    def train_weights(self, handle):
        out, ptrs = self._weight_outs()
        self._chk(lib().ck_train_get_weights(self._h, int(handle), ptrs))
        return out

    def train_adam_state(self, handle):
        """-> (first moments, second moments, updates applied)"""
        m, mp = self._weight_outs()
        v, vp = self._weight_outs()
        steps = C.c_longlong(0)
        self._chk(lib().ck_train_get_adam_state(self._h, int(handle), mp, vp, C.byref(steps)))
        return m, v, int(steps.value)

    def train_handover(self, handle):
        """the trainer's current weights become the context's classifier (no host round trip)"""
        self._chk(lib().ck_train_handover(self._h, int(handle)))

    # ---- training data from goban images (csrc/k_harvest.hip) ------------------------------------------------
    def harvest_patches(self, goban, fgcount, state_of, positions, calm_max=16, empty_keep=256, seed=0, first_frame=0, cap=None):
        """the labelled regions of n goban images (n, 380, 380, 3), host or device: region q of frame i is kept when
        state_of[i] >= 0 (an index into positions (n_pos, 19, 19), codes 0 / 1 / 2), the foreground counts fgcount (n, 19, 19)
        of its four zones sum to <= calm_max and, if its label is 0, the hash of (seed, first_frame + i, q) lets it through
        (empty_keep of 256).  -> (x (k, 40, 40, 3) uint8, labels (k,) uint8, src (k, 2) int32 = (frame, region)) in ascending
        (frame, region) order, where goban lies; at most `cap` of them (default: room for all n * 100)"""
        shp = tuple(int(v) for v in goban.shape)
        if len(shp) == 3:
            shp = (1,) + shp
        if len(shp) != 4 or shp[1:] != (380, 380, 3):
            raise ValueError("goban images (n, 380, 380, 3) expected, got %r" % (tuple(goban.shape),))
        n = shp[0]
        state = np.ascontiguousarray(state_of, np.int32).reshape(-1)
        pos = np.ascontiguousarray(positions, np.uint8).reshape(-1, 361)
        if len(state) != n or tuple(fgcount.shape) not in ((n, 19, 19), (n, 361)):
            raise ValueError("%d frames with %d states and counts %r" % (n, len(state), tuple(fgcount.shape)))
        cap = n * 100 if cap is None else int(cap)
        if _is_torch(goban):
            goban = goban.contiguous()
        if _is_torch(fgcount):
            fgcount = fgcount.contiguous()
        room = max(cap, 0)
        x, xp, osp = self._out(goban, (room, 40, 40, 3), np.uint8)
        lab, lp, _ = self._out(goban, (room,), np.uint8)
        src, sp_, _ = self._out(goban, (room, 2), np.int32)
        p, sp, keep = self._in(goban, what="goban")
        fp, fsp, fkeep = self._in(fgcount, np.int32, what="fgcount")
        found = C.c_int32(0)
        self._chk(lib().ck_harvest_patches(self._h, p, n, sp, fp, fsp, state.ctypes.data_as(C.c_void_p),
                                           pos.ctypes.data_as(C.c_void_p), len(pos), int(calm_max), int(empty_keep),
                                           int(seed) & 0xffffffff, int(first_frame), xp, lp, sp_, cap, osp, C.byref(found)))
        self.harvest_found = int(found.value)                # the total, also when cap cut the outputs short
        k = min(self.harvest_found, room)
        return x[:k], lab[:k], src[:k]

    def augment_patches(self, x, t, to_device=None, out=None):
        """x (n, 40, 40, 3) uint8, host or device; t: n codes 0..7 -> numpy.rot90(x[k], t[k] & 3), its columns mirrored when
        t[k] & 4, as a new array where x lies -- or a device tensor on `to_device`, or written into `out`"""
        shp = tuple(int(v) for v in x.shape)
        if len(shp) != 4 or shp[1:] != (40, 40, 3):
            raise ValueError("patches (n, 40, 40, 3) expected, got %r" % (shp,))
        n = shp[0]
        if _is_torch(t):
            t = t.detach().cpu().numpy()
        t = np.asarray(t).reshape(-1)
        if len(t) != n:
            raise ValueError("%d transform codes for %d patches" % (len(t), n))
        codes = np.ascontiguousarray(np.where((t < 0) | (t > 255), 255, t), np.uint8)       # out of range: the library says so
        if _is_torch(x):
            x = x.contiguous()
        if out is not None and tuple(out.shape) != shp:
            raise ValueError("out %r for patches %r" % (tuple(out.shape), shp))
        res, op, osp = self._out(x, shp, np.uint8, out, to_device)
        p, sp, keep = self._in(x, what="x")
        self._chk(lib().ck_augment_patches(self._h, p, n, sp, codes.ctypes.data_as(C.c_void_p), op, osp))
        return res

    def stones_detect(self, bgr, M):
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        M = np.ascontiguousarray(M, np.float64).reshape(-1, 9)
        labels, lp, osp = self._out(bgr, (n, 19, 19), np.uint8)
        conf, cp, _ = self._out(bgr, (n, 19, 19), np.float64)
        self._chk(lib().ck_stones_detect(self._h, p, n, h, w, sp, M.ctypes.data_as(C.c_void_p), len(M), lp, cp, osp))
        return labels, conf

    # ---- ordered stones path (feeds PolicyCore) ---------------------------------------------------
    def cnn_regions(self, goban):
        """-> (region_label (n, 10, 10) uint8, region_conf (n, 10, 10) float64)"""
        n, p, sp, keep = self._goban(goban)
        rl, rlp, osp = self._out(goban, (n, 10, 10), np.uint8)
        rc, rcp, _ = self._out(goban, (n, 10, 10), np.float64)
        self._chk(lib().ck_cnn_regions(self._h, p, n, sp, rlp, rcp, osp))
        return rl, rc

    def stones_run(self, bgr, M, mog2=None, learning_rates=None, want_grid=False):
        """ordered run of n consecutive frames of one stream -> dict(region_label, region_conf, fgcount[, labels, conf]);
        fgcount is None without a background model"""
        n, h, w = self._shape(bgr, 3)
        p, sp, keep = self._in(bgr)
        M = np.ascontiguousarray(M, np.float64).reshape(-1, 9)
        rl, rlp, osp = self._out(bgr, (n, 10, 10), np.uint8)
        rc, rcp, _ = self._out(bgr, (n, 10, 10), np.float64)
        fg, fgp, lr, lrp = None, None, None, None
        if mog2 is not None:
            fg, fgp, _ = self._out(bgr, (n, 19, 19), np.int32)
            lr = np.ascontiguousarray(learning_rates, np.float64).reshape(n)
            lrp = lr.ctypes.data_as(C.c_void_p)
        lab, labp, cf, cfp = None, None, None, None
        if want_grid:
            lab, labp, _ = self._out(bgr, (n, 19, 19), np.uint8)
            cf, cfp, _ = self._out(bgr, (n, 19, 19), np.float64)
        self._chk(lib().ck_stones_run(self._h, p, n, h, w, sp, M.ctypes.data_as(C.c_void_p), len(M),
                                      -1 if mog2 is None else int(mog2), lrp, rlp, rcp, fgp, labp, cfp, osp))
        return dict(region_label=rl, region_conf=rc, fgcount=fg, labels=lab, conf=cf)

    def mog2_band_run(self, handle, band, learning_rates, last_band):
        """band (n, band_h, 380, 3) of consecutive goban images -> int32 (n, zone rows, 19) foreground counts"""
        h, w = self._mog2_hw(handle)                 # (the library reads n bands of the MODEL's size and writes its zone rows)
        n = int(band.shape[0])
        p, sp, keep = self._in(band, np.uint8, (n, h, w, 3), "band")
        lr = np.ascontiguousarray(learning_rates, np.float64).reshape(n)
        out, op, osp = self._out(band, (n, (h + 19) // 20, 19), np.int32)
        self._chk(lib().ck_mog2_band_run(self._h, int(handle), p, n, sp, lr.ctypes.data_as(C.c_void_p), int(bool(last_band)),
                                         op, osp))
        return out

    def zone_counts(self, mask):
        """(n, 380, 380) or (380, 380) mask -> int32 (n, 19, 19) / (19, 19) foreground pixels per intersection zone"""
        single = len(mask.shape) == 2
        n = _batch_of(mask, (380, 380), "mask")
        p, sp, keep = self._in(mask, what="mask")
        out, op, osp = self._out(mask, (19, 19) if single else (n, 19, 19), np.int32)
        self._chk(lib().ck_zone_counts(self._h, p, n, sp, op, osp))
        return out

    # ---- SfContours.find_stones -------------------------------------------------------------
    def contour_stones(self, goban, fg, rects, rs=0, re=19, cs=0, ce=19, want_all=False):
        """SfContours.find_stones (stone/sf_contours.py:48-111) for one goban image (side, side, 3) + its foreground mask
        (side, side), or a batch (n, ...) of them, host or device; rects = (19, 19, 4) StonesFinder.getrect table.
        -> stones uint8 (19, 19) / (n, 19, 19) of 0 E, 1 B, 2 W (and with want_all: zones int16 (.., re-rs, ce-cs, 4),
        the hull mask uint8 (.., hs, ws) of the analysed view)"""
        single = len(goban.shape) == 3
        n = 1 if single else int(goban.shape[0])
        side = int(goban.shape[-2])
        if tuple(goban.shape[-3:]) != (side, side, 3) or tuple(fg.shape[-2:]) != (side, side) or len(fg.shape) != len(goban.shape) - 1:
            raise ValueError("goban %r / foreground %r: expected (.., s, s, 3) and (.., s, s)" % (tuple(goban.shape), tuple(fg.shape)))
        rects = np.ascontiguousarray(rects, np.int32).reshape(19, 19, 4)
        p, sp, keep = self._in(goban)
        q, sq, keep2 = self._in(fg)
        if sp != sq:
            raise ValueError("goban image and foreground mask must live in the same space (both host or both device)")
        stones = np.zeros((n, 19, 19), np.uint8)
        zones = mask = None
        zp = mp = None
        if want_all:
            hs = int(rects[re - 1, ce - 1, 2] - rects[rs, cs, 0])
            ws = int(rects[re - 1, ce - 1, 3] - rects[rs, cs, 1])
            zones = np.zeros((n, re - rs, ce - cs, 4), np.int16)
            mask = np.zeros((n, max(hs, 0), max(ws, 0)), np.uint8)
            zp, mp = zones.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)
        self._chk(lib().ck_contour_stones(self._h, p, q, n, side, sp, rects.ctypes.data_as(C.c_void_p), int(rs), int(re), int(cs),
                                          int(ce), stones.ctypes.data_as(C.c_void_p), zp, mp))
        if single:
            return (stones[0], zones[0], mask[0]) if want_all else stones[0]
        return (stones, zones, mask) if want_all else stones

    def cluster_stones(self, goban, rects, mask, jobs=None, rs=0, re=19, cs=0, ce=19, want_all=False):
        """SfClustering.find_stones (stone/sf_clustering.py:48-168) for a list of jobs in one call (ck_cluster_stones).
        goban: one image (side, side, 3) or a batch (n, side, side, 3), uint8 or float32, host or device; rects: the
        (19, 19, 4) getrect table; mask: (side, side) StonesFinder.getmask(); jobs: (m, 5) rows of (image, rs, re, cs, ce) --
        None: one job per image over rows [rs, re) x columns [cs, ce).
        -> stones uint8 (m, 19, 19) of 0 E / 1 B / 2 W, trusted bool (m,) -- for one image and jobs=None: (19, 19) and a bool.
        want_all: also a dict of ratios (m, 19, 19, 3), centers (m, 3, 3), labels (list of (hs, ws) uint8 arrays), passes
        (m, 3), compactness (m, 3), winner (m,).  Each job draws 21 numbers from the context's generator (`rng_state`)."""
        single = len(goban.shape) == 3
        n = 1 if single else int(goban.shape[0])
        side = int(goban.shape[-2])
        if tuple(goban.shape[-3:]) != (side, side, 3):
            raise ValueError("goban %r: expected (.., s, s, 3)" % (tuple(goban.shape),))
        is_f32 = "float32" in str(goban.dtype)
        if not is_f32 and "uint8" not in str(goban.dtype):
            raise ValueError("goban images are uint8 or float32, not %s" % goban.dtype)
        rects = np.ascontiguousarray(rects, np.int32).reshape(19, 19, 4)
        mask = np.ascontiguousarray(mask, np.uint8)
        if mask.shape != (side, side):
            raise ValueError("mask %r: expected (%d, %d)" % (mask.shape, side, side))
        plain = jobs is None
        if plain:
            jobs = [(f, rs, re, cs, ce) for f in range(n)]
        jobs = np.ascontiguousarray(jobs, np.int32).reshape(-1, 5)
        m = len(jobs)
        p, sp, keep = self._in(goban, np.float32 if is_f32 else np.uint8)
        stones = np.zeros((m, 19, 19), np.uint8)
        trusted = np.zeros(m, np.uint8)
        extra, ptrs, cap = {}, [None] * 3 + [0] + [None] * 3, 0
        if want_all:
            views = []
            for f, a, b, c, d in jobs:                  # (a bad job is refused by the library; sizes here only bound the buffer)
                ok = 0 <= a < b <= 19 and 0 <= c < d <= 19
                views.append((max(int(rects[b - 1, d - 1, 2] - rects[a, c, 0]), 0), max(int(rects[b - 1, d - 1, 3] - rects[a, c, 1]), 0)) if ok else (0, 0))
            cap = sum(h * w for h, w in views)
            extra = dict(ratios=np.zeros((m, 19, 19, 3), np.uint8), centers=np.zeros((m, 3, 3), np.float32),
                         labels=np.zeros(max(cap, 1), np.uint8), passes=np.zeros((m, 3), np.int32),
                         compactness=np.zeros((m, 3), np.float64), winner=np.zeros(m, np.int32))
            ptrs = [extra[k].ctypes.data_as(C.c_void_p) for k in ("ratios", "centers", "labels")] + [cap] + \
                   [extra[k].ctypes.data_as(C.c_void_p) for k in ("passes", "compactness", "winner")]
        self._chk(lib().ck_cluster_stones(self._h, p, n, side, int(is_f32), sp, rects.ctypes.data_as(C.c_void_p),
                                          mask.ctypes.data_as(C.c_void_p), jobs.ctypes.data_as(C.c_void_p), m,
                                          stones.ctypes.data_as(C.c_void_p), trusted.ctypes.data_as(C.c_void_p), *ptrs))
        trusted = trusted.astype(bool)
        if want_all:
            flat, off, extra["labels"] = extra["labels"], 0, []
            for h, w in views:
                extra["labels"].append(flat[off:off + h * w].reshape(h, w))
                off += h * w
        if single and plain:
            stones, trusted = stones[0], bool(trusted[0])
        return (stones, trusted, extra) if want_all else (stones, trusted)

    @property
    def rng_state(self):
        """the cv::RNG state the context's k-means draws from (64 bits; a fresh context holds 0xffffffff)"""
        v = C.c_uint64(0)
        self._chk(lib().ck_rng_get(self._h, C.byref(v)))
        return int(v.value)

    @rng_state.setter
    def rng_state(self, state):
        self._chk(lib().ck_rng_set(self._h, int(state) & 0xffffffffffffffff))

    def contours_external(self, edges, want_points=False):
        """cv2.findContours(edges, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) as SfContours reads it: for one (h, w) edge map or a
        batch (n, h, w) -> per map a list of dicts {start: (x, y), nvert, pix: (k, 2) int32 or None} in cv2's order"""
        single = len(edges.shape) == 2
        n = 1 if single else int(edges.shape[0])
        h, w = int(edges.shape[-2]), int(edges.shape[-1])
        p, sp, keep = self._in(edges)
        cap = n * (h * w // 4 + 1)
        counts = np.zeros(n, np.int32)
        table = np.zeros((cap, 4), np.int32)
        pts = np.zeros((n * h * w, 2), np.int32) if want_points else None
        self._chk(lib().ck_contours_external(self._h, p, n, h, w, sp, counts.ctypes.data_as(C.c_void_p),
                                             table.ctypes.data_as(C.c_void_p), cap,
                                             pts.ctypes.data_as(C.c_void_p) if want_points else None, n * h * w))
        out, k, o = [], 0, 0
        for f in range(n):
            lst = []
            for _ in range(int(counts[f])):
                x, y, nv, npx = (int(v) for v in table[k])
                lst.append(dict(start=(x, y), nvert=nv, pix=pts[o:o + npx].copy() if want_points else None))
                k += 1
                o += npx
            out.append(lst)
        return out[0] if single else out

    # ---- StonesFinder.find_intersections ----------------------------------------------------
    def find_intersections(self, goban, mtx, rects, want_lines=False):
        """StonesFinder.find_intersections (stone/stonesfinder.py:516-552) for one goban image (side, side, 3) or a batch,
        host or device; mtx (19, 19, 2) int16 PosGrid.mtx, rects (19, 19, 4) getrect table -> grid int16 (.., 19, 19, 2)
        (with want_lines also: per image a dict {(r, c): [(x0, y0, x1, y1), ..]} of the lines found, and the Canny map)"""
        single = len(goban.shape) == 3
        n = 1 if single else int(goban.shape[0])
        side = int(goban.shape[-2])
        if tuple(goban.shape[-3:]) != (side, side, 3):
            raise ValueError("goban %r: expected (.., s, s, 3)" % (tuple(goban.shape),))
        mtx = np.ascontiguousarray(mtx, np.int16).reshape(19, 19, 2)
        rects = np.ascontiguousarray(rects, np.int32).reshape(19, 19, 4)
        p, sp, keep = self._in(goban)
        grid = np.zeros((n, 19, 19, 2), np.int16)
        lines = counts = edges = None
        lp = cp = ep = None
        if want_lines:
            lines = np.zeros((n, 361, ZONE_LINES, 4), np.int16)
            counts = np.zeros((n, 361), np.int32)
            edges = np.zeros((n, side, side), np.uint8)
            lp, cp, ep = (a.ctypes.data_as(C.c_void_p) for a in (lines, counts, edges))
        self._chk(lib().ck_find_intersections(self._h, p, n, side, sp, mtx.ctypes.data_as(C.c_void_p), rects.ctypes.data_as(C.c_void_p),
                                              grid.ctypes.data_as(C.c_void_p), lp, cp, ep))
        if not want_lines:
            return grid[0] if single else grid
        found = [{divmod(z, 19): [tuple(int(v) for v in lines[f, z, k]) for k in range(counts[f, z])]
                  for z in np.nonzero(counts[f])[0]} for f in range(n)]
        return (grid[0], found[0], edges[0]) if single else (grid, found, edges)


def _host_error(rc):
    err = CkError("libck_hip error %d: %s" % (rc, (lib().ck_last_error(None) or b"").decode()))
    err.code = rc
    return err


def jpeg_blocks(h, w, sampling):
    """8x8 blocks of one frame, all components, on the MCU-padded grid (ck_jpeg_info.blocks)"""
    if sampling not in (CK_JPEG_GREY, CK_JPEG_444, CK_JPEG_422, CK_JPEG_420) or h <= 0 or w <= 0:
        raise CkError("bad JPEG geometry %dx%d sampling %r" % (w, h, sampling))
    hs, vs = (2 if sampling >= CK_JPEG_422 else 1), (2 if sampling == CK_JPEG_420 else 1)
    return -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + (0 if sampling == CK_JPEG_GREY else 2))


def _jpeg_streams(streams):
    """-> (array of pointers, array of lengths, the uint8 arrays that own the bytes)"""
    keep = [np.ascontiguousarray(np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray, memoryview)) else s, np.uint8).reshape(-1)
            for s in streams]
    if not keep:
        raise CkError("no JPEG stream given")
    ptrs = (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    lens = (C.c_size_t * len(keep))(*[a.size for a in keep])
    return ptrs, lens, keep


def _jpeg_probe(stream):
    """-> (status, dict or None, the library's message)"""
    ptrs, lens, keep = _jpeg_streams([stream])
    info = JpegInfo()
    rc = lib().ck_jpeg_probe(C.c_void_p(keep[0].ctypes.data), keep[0].size, C.byref(info))
    if rc != 0:
        return rc, None, (lib().ck_last_error(None) or b"").decode()
    return 0, dict(h=info.h, w=info.w, sampling=info.sampling, restart_interval=info.restart_interval, blocks=info.blocks), ""


def jpeg_probe(stream):
    """the headers of one baseline JPEG stream -> dict(h, w, sampling (CK_JPEG_*), restart_interval, blocks); host only.
    CkError (code CK_ERR_DATA) for a stream the decoder refuses, with the cause."""
    rc, info, why = _jpeg_probe(stream)
    if rc != 0:
        err = CkError("libck_hip error %d: %s" % (rc, why))
        err.code = rc
        raise err
    return info


def jpeg_coefficients(streams):
    """the Huffman stage alone (host only): streams of one geometry -> (info of the first, coef (n, blocks * 64) int16,
    quant (n, 3, 64) uint16) in the layout of ck_jpeg_coefficients.  CkError (CK_ERR_DATA) names the frame that failed;
    its index is the error's `bad_frame`."""
    ptrs, lens, keep = _jpeg_streams(streams)
    n = len(keep)
    info = jpeg_probe(keep[0])
    geom = JpegInfo(info["h"], info["w"], info["sampling"], info["restart_interval"], info["blocks"])
    coef = np.empty((n, info["blocks"] * 64), np.int16)
    quant = np.empty((n, 3, 64), np.uint16)
    bad = C.c_int32(-1)
    rc = lib().ck_jpeg_coefficients(ptrs, lens, n, C.byref(geom), coef.ctypes.data_as(C.c_void_p),
                                    quant.ctypes.data_as(C.c_void_p), C.byref(bad))
    if rc != 0:
        err = _host_error(rc)
        err.bad_frame = bad.value
        raise err
    return info, coef, quant


def jpeg_plan(streams):
    """the plan of the strand decoder (host only): streams of one geometry -> (rows (strands, 6) int64 of {frame, begin, end,
    first_mcu, n_mcu, table_set}, the number of table sets).  A strand is one restart interval of one frame, begin / end
    byte offsets into its stream.  CkError (CK_ERR_DATA) names the frame that was refused."""
    ptrs, lens, keep = _jpeg_streams(streams)
    n = len(keep)
    info = jpeg_probe(keep[0])
    geom = JpegInfo(info["h"], info["w"], info["sampling"], info["restart_interval"], info["blocks"])
    count, sets, bad = C.c_longlong(0), C.c_int32(0), C.c_int32(-1)
    rows = np.empty((0, 6), np.int64)
    for _ in range(2):                                   # (the first call sizes the array)
        _check_array(rows, (rows.shape[0], 6), np.int64, "strands", writeable=True)
        rc = lib().ck_jpeg_plan(ptrs, lens, n, C.byref(geom), rows.ctypes.data_as(C.c_void_p), rows.shape[0],
                                C.byref(count), C.byref(sets), C.byref(bad))
        if rc != CK_ERR_CAPACITY:
            break
        rows = np.empty((count.value, 6), np.int64)
    if rc != 0:
        err = _host_error(rc)
        if bad.value >= 0:
            err.bad_frame = bad.value
        raise err
    return rows[:count.value], sets.value


def jpeg_coefficients_strands(streams):
    """jpeg_coefficients through the plan and the strand decoder the GPU kernel runs, on the host (host only): the same
    results, the same accept / refuse decisions"""
    ptrs, lens, keep = _jpeg_streams(streams)
    n = len(keep)
    info = jpeg_probe(keep[0])
    geom = JpegInfo(info["h"], info["w"], info["sampling"], info["restart_interval"], info["blocks"])
    coef = np.empty((n, info["blocks"] * 64), np.int16)
    quant = np.empty((n, 3, 64), np.uint16)
    bad = C.c_int32(-1)
    rc = lib().ck_jpeg_coefficients_strands(ptrs, lens, n, C.byref(geom), coef.ctypes.data_as(C.c_void_p),
                                            quant.ctypes.data_as(C.c_void_p), C.byref(bad))
    if rc != 0:
        err = _host_error(rc)
        err.bad_frame = bad.value
        raise err
    return info, coef, quant


JPEG_SPAN_STATS = ("spans", "unresolved", "suspect_strands", "one_lane_frames")


def jpeg_span_bytes():
    """the default span size of the "device-spans" entropy mode, in bytes"""
    b = C.c_int32(0)
    rc = lib().ck_jpeg_span_bytes(C.byref(b))
    if rc != 0:
        raise _host_error(rc)
    return b.value


def jpeg_coefficients_spans(streams, span_bytes=None):
    """jpeg_coefficients through the steps the "device-spans" kernels run (speculate, resolve, write, dc, verdict, and the
    one-lane decoder for suspect frames), on the host (host only) -> (info, coef, quant, stats): the same results, the same
    accept / refuse decisions; stats as Context.jpeg_span_stats gives them (also the error's `stats` on a refusal)"""
    ptrs, lens, keep = _jpeg_streams(streams)
    n = len(keep)
    info = jpeg_probe(keep[0])
    geom = JpegInfo(info["h"], info["w"], info["sampling"], info["restart_interval"], info["blocks"])
    coef = np.empty((n, info["blocks"] * 64), np.int16)
    quant = np.empty((n, 3, 64), np.uint16)
    bad = C.c_int32(-1)
    st = (C.c_longlong * 4)()
    rc = lib().ck_jpeg_coefficients_spans(ptrs, lens, n, C.byref(geom), jpeg_span_bytes() if span_bytes is None else int(span_bytes),
                                          coef.ctypes.data_as(C.c_void_p), quant.ctypes.data_as(C.c_void_p), C.byref(bad), st)
    stats = dict(zip(JPEG_SPAN_STATS, (int(v) for v in st)))
    if rc != 0:
        err = _host_error(rc)
        err.bad_frame = bad.value
        err.stats = stats
        raise err
    return info, coef, quant, stats


def _check_frames(frames):
    shp = tuple(frames.shape)
    name = str(frames.dtype).replace("torch.", "")
    if len(shp) not in (3, 4) or shp[-1] != 3 or name != "uint8" or 0 in shp:
        raise CkError("frames: a uint8 array of shape (n, h, w, 3) or (h, w, 3) is needed, got %s %r" % (name, shp))
    if _is_torch(frames) and not frames.is_contiguous():
        raise CkError("frames: a contiguous tensor is needed")


def _quant_tables(quant):
    quant = np.ascontiguousarray(quant, np.uint16)
    if quant.shape != (3, 64):
        raise CkError("quant: tables of shape (3, 64) are needed, got %r" % (quant.shape,))
    return quant


def jpeg_quant(quality):
    """the quant tables libjpeg derives from a quality (clamped to 1 .. 100) -> (3, 64) uint16, natural order, by
    component (Y, Cb, Cr); host only"""
    quant = np.empty((3, 64), np.uint16)
    rc = lib().ck_jpeg_quant(int(quality), quant.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise _host_error(rc)
    return quant


def jpeg_encode_bound(h, w, sampling):
    """the largest stream a frame of h x w can become, in bytes; host only"""
    b = C.c_size_t(0)
    rc = lib().ck_jpeg_encode_bound(int(h), int(w), int(sampling), C.byref(b))
    if rc != 0:
        raise _host_error(rc)
    return b.value


def jpeg_entropy_encode(coef, quant, h, w, sampling, restart_interval=0, optimize=False):
    """the Huffman stage of the encoder alone (host only): coefficients (n, blocks * 64) int16, or (blocks * 64,) of one
    frame, in the layout of jpeg_coefficients + one set of quant tables (3, 64) -> a list of n `bytes` (one `bytes` for one
    frame).  CkError (CK_ERR_ARG) for a coefficient the baseline Huffman tables cannot code.  optimize=True: tables fitted
    to each frame (ck_jpeg_entropy_encode_opt), the bytes of PIL's optimize=True."""
    h, w, sampling = int(h), int(w), int(sampling)
    coef = np.ascontiguousarray(coef, np.int16)
    single = coef.ndim == 1
    coef = coef.reshape(1, -1) if single else coef
    n = coef.shape[0]
    _check_array(coef, (n, jpeg_blocks(h, w, sampling) * 64), np.int16, "coef")
    quant = _quant_tables(quant)
    stride = jpeg_encode_bound(h, w, sampling)
    out = np.empty(max(1, n) * stride, np.uint8)
    lens = (C.c_size_t * max(1, n))()
    fn = lib().ck_jpeg_entropy_encode_opt if optimize else lib().ck_jpeg_entropy_encode
    rc = fn(coef.ctypes.data_as(C.c_void_p), quant.ctypes.data_as(C.c_void_p), n, h, w, sampling,
            int(restart_interval), out.ctypes.data_as(C.c_void_p), stride, lens)
    if rc != 0:
        raise _host_error(rc)
    streams = [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)]
    return streams[0] if single else streams


def jpeg_entropy_encode_staged(coef, quant, h, w, sampling, restart_interval=0, optimize=False):
    """jpeg_entropy_encode through the steps the GPU kernels run (size, scan, put, stuff; with optimize=True histo and tables
    in front of them), on the host (host only): the same streams, the same refusals"""
    h, w, sampling = int(h), int(w), int(sampling)
    coef = np.ascontiguousarray(coef, np.int16)
    single = coef.ndim == 1
    coef = coef.reshape(1, -1) if single else coef
    n = coef.shape[0]
    _check_array(coef, (n, jpeg_blocks(h, w, sampling) * 64), np.int16, "coef")
    quant = _quant_tables(quant)
    stride = jpeg_encode_bound(h, w, sampling)
    out = np.empty(max(1, n) * stride, np.uint8)
    lens = (C.c_size_t * max(1, n))()
    fn = lib().ck_jpeg_entropy_encode_opt_staged if optimize else lib().ck_jpeg_entropy_encode_staged
    rc = fn(coef.ctypes.data_as(C.c_void_p), quant.ctypes.data_as(C.c_void_p), n, h, w, sampling,
            int(restart_interval), out.ctypes.data_as(C.c_void_p), stride, lens)
    if rc != 0:
        raise _host_error(rc)
    streams = [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)]
    return streams[0] if single else streams


def jpeg_histogram(coef, h, w, sampling, restart_interval=0):
    """the symbols the Huffman coder emits for each frame, counted (host only): coefficients (n, blocks * 64) int16, or
    (blocks * 64,) of one frame -> (n, 4, 256) uint32, or (4, 256): DC luma, AC luma, DC chroma, AC chroma, the order of the
    DHT segments.  CkError for a coefficient the coder refuses."""
    h, w, sampling = int(h), int(w), int(sampling)
    coef = np.ascontiguousarray(coef, np.int16)
    single = coef.ndim == 1
    coef = coef.reshape(1, -1) if single else coef
    n = coef.shape[0]
    _check_array(coef, (n, jpeg_blocks(h, w, sampling) * 64), np.int16, "coef")
    counts = np.zeros((max(1, n), 4, 256), np.uint32)
    rc = lib().ck_jpeg_histogram(coef.ctypes.data_as(C.c_void_p), n, h, w, sampling, int(restart_interval), counts.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise _host_error(rc)
    return counts[0] if single else counts[:n]


def jpeg_optimal_table(counts):
    """libjpeg's jpeg_gen_optimal_table (host only): 256 symbol counts -> (bits, vals): bits (16,) uint8, the number of codes
    of 1 .. 16 bits, and the symbols in the order of their codes -- the body of a DHT segment"""
    counts = np.ascontiguousarray(counts, np.uint32)
    _check_array(counts, (256,), np.uint32, "counts")
    bits, vals, count = np.zeros(16, np.uint8), np.zeros(256, np.uint8), C.c_int32(0)
    rc = lib().ck_jpeg_optimal_table(counts.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p),
                                     C.byref(count))
    if rc != 0:
        raise _host_error(rc)
    return bits, vals[:count.value].copy()


def jpeg_enc_tiles():
    """(blocks, bytes): how many blocks in scan order one workgroup of the GPU Huffman coder assembles, how many unstuffed
    bytes one places; host only"""
    b, y = C.c_int32(0), C.c_int32(0)
    rc = lib().ck_jpeg_enc_tiles(C.byref(b), C.byref(y))
    if rc != 0:
        raise _host_error(rc)
    return b.value, y.value


def _png_info(stream, deep):
    ptrs, lens, keep = _jpeg_streams([stream])
    info = PngInfo()
    fn = lib().ck_png_probe if deep else lib().ck_png_header
    rc = fn(C.c_void_p(keep[0].ctypes.data), keep[0].size, C.byref(info))
    if rc != 0:
        raise _host_error(rc)
    return dict(h=info.h, w=info.w, color_type=info.color_type, bit_depth=info.bit_depth, palette_entries=info.palette_entries,
                rowbytes=info.rowbytes)


def png_header(stream):
    """the chunk walk of one PNG file alone (signature, CRCs, IHDR) -> dict(h, w, color_type, bit_depth, palette_entries,
    rowbytes); host only.  CkError (code CK_ERR_DATA) with the cause for a file the reader refuses."""
    return _png_info(stream, False)


def png_probe(stream):
    """everything the host does for one PNG file -- the chunk walk, the inflate, the size of its output, the filter bytes --
    -> the dict of png_header; host only.  CkError (code CK_ERR_DATA) with the cause for a file the reader refuses."""
    return _png_info(stream, True)


def png_inflate(data):
    """a zlib stream -> its bytes, by the library's own inflate (host only): what zlib.decompress gives, and CkError (code
    CK_ERR_DATA) where zlib.decompress raises"""
    ptrs, lens, keep = _jpeg_streams([data])
    cap = max(1 << 16, 8 * keep[0].size)
    while True:
        out = np.empty(cap, np.uint8)
        total = C.c_size_t(0)
        rc = lib().ck_png_inflate(C.c_void_p(keep[0].ctypes.data), keep[0].size, out.ctypes.data_as(C.c_void_p), cap, C.byref(total))
        if rc != 0:
            raise _host_error(rc)
        if total.value <= cap:
            return out[:total.value].tobytes()
        cap = total.value


def png_inflate_staged(data, cap=None, rows=None, verdict=False):
    """png_inflate through the steps of the device inflate in plain loops on the host, in the kernel's order (host only): the
    same bytes, and CkError with the same message.  cap: keep only the first `cap` bytes (None: all).  rows: (h, rowbytes) --
    the stream holds h rows of 1 + rowbytes bytes, and the PNG reader's two checks (enough bytes, filter bytes up to 4)
    follow the inflate.  verdict=True: no error is raised; -> dict(data (None for a refused stream), total, cause,
    produced, message)"""
    ptrs, lens, keep = _jpeg_streams([data])
    h, rowbytes = (0, 0) if rows is None else (int(rows[0]), int(rows[1]))
    room = max(1 << 16, 8 * keep[0].size) if cap is None else int(cap)
    while True:
        out = np.empty(max(room, 1), np.uint8)
        total, cause, produced = C.c_size_t(0), C.c_int32(0), C.c_longlong(0)
        rc = lib().ck_png_inflate_staged(C.c_void_p(keep[0].ctypes.data), keep[0].size, out.ctypes.data_as(C.c_void_p), room, C.byref(total),
                                         h, rowbytes, C.byref(cause), C.byref(produced))
        if rc != 0 and (not verdict or rc != CK_ERR_DATA):
            raise _host_error(rc)
        if rc == 0 and cap is None and total.value > room:
            room = total.value
            continue
        got = None if rc else out[:min(room, total.value)].tobytes()
        if not verdict:
            return got
        return dict(data=got, total=total.value, cause=cause.value, produced=produced.value,
                    message=(lib().ck_last_error(None) or b"").decode() if rc else "")


def png_inflate_geometry():
    """the seams of the inflate kernel -> dict(window_bits: the bit offsets a window step decodes at once; flush_bytes: the
    bytes that leave the ring of 2 * flush_bytes at a time); host only"""
    v = [C.c_int32(0) for _ in range(2)]
    rc = lib().ck_png_inflate_geometry(*[C.byref(x) for x in v])
    if rc != 0:
        raise _host_error(rc)
    return dict(window_bits=v[0].value, flush_bytes=v[1].value)


def png_encode_bound(h, w):
    """the largest file a frame of h x w can become, in bytes; host only"""
    b = C.c_size_t(0)
    rc = lib().ck_png_encode_bound(int(h), int(w), C.byref(b))
    if rc != 0:
        raise _host_error(rc)
    return b.value


def _png_filter(filter):
    if filter is None:
        return -1
    if filter not in (0, 1, 2, 3, 4):
        raise CkError("png filter: None (chosen per row) or 0 .. 4 (None, Sub, Up, Avg, Paeth) is needed, got %r" % (filter,))
    return int(filter)


def png_encode_staged(frames, filter=None, runs=False):
    """Context.png_encode through the same steps in plain loops on the host (host only): BGR frames (n, h, w, 3) or one
    frame (h, w, 3) -> a list of n `bytes`, byte for byte what the GPU writes.  runs: False the literal-only mode, True the
    runs mode, or one of CK_PNG_MATCH_*"""
    if not isinstance(runs, (bool, int, np.integer)):
        raise CkError("png runs: True, False or one of CK_PNG_MATCH_* is needed, got %r" % (runs,))
    _check_frames(frames)
    frames = np.ascontiguousarray(frames.numpy() if _is_torch(frames) else frames, np.uint8)
    n, h, w = Context._shape(frames, 3)
    stride = png_encode_bound(h, w)
    out = np.empty(n * stride, np.uint8)
    lens = (C.c_size_t * n)()
    if runs is False:
        rc = lib().ck_png_encode_staged(frames.ctypes.data_as(C.c_void_p), n, h, w, _png_filter(filter), out.ctypes.data_as(C.c_void_p), stride, lens)
    else:
        rc = lib().ck_png_encode_staged_mode(frames.ctypes.data_as(C.c_void_p), n, h, w, _png_filter(filter), int(runs),
                                             out.ctypes.data_as(C.c_void_p), stride, lens)
    if rc != 0:
        raise _host_error(rc)
    return [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)]


def png_tiles():
    """the seams of the PNG kernels -> dict(band_rows, tile_bytes: the encoder's deflate block and bit-packing tile;
    chunk_bytes, group_rows: what a lane of the unfilter kernel takes per step and the rows in flight); host only"""
    v = [C.c_int32(0) for _ in range(4)]
    rc = lib().ck_png_tiles(*[C.byref(x) for x in v])
    if rc != 0:
        raise _host_error(rc)
    return dict(zip(("band_rows", "tile_bytes", "chunk_bytes", "group_rows"), (x.value for x in v)))


def overlay_plan(n, h, w, prims, frame_start, text_len=0):
    """the plan ck_overlay_draw runs for n images of h x w (host only): prims (P, 8) int32, frame_start (n + 1,) int32 as
    core.overlay.pack gives them -> (bin_size, bin_start (n * bins + 1,), bin_prims): bin b of the images, cut into squares
    of bin_size row by row and frame after frame, owns bin_prims[bin_start[b]:bin_start[b + 1]], the indices of the
    primitives whose bounding box meets it, ascending.  CkError (CK_ERR_ARG) for a list outside the limits."""
    n, h, w = int(n), int(h), int(w)
    prims = np.ascontiguousarray(prims, np.int32).reshape(-1, 8)
    frame_start = np.ascontiguousarray(frame_start, np.int32)
    if frame_start.shape != (n + 1,) or (n > 0 and int(frame_start.max()) > len(prims)):
        raise CkError("frame_start: %d + 1 offsets into the %d primitives are needed" % (n, len(prims)))
    bin_size, n_refs = C.c_int32(0), C.c_int32(0)
    args = (n, h, w, prims.ctypes.data_as(C.c_void_p), frame_start.ctypes.data_as(C.c_void_p), int(text_len), C.byref(bin_size))
    rc = lib().ck_overlay_plan(*args, None, None, 0, C.byref(n_refs))
    if rc != 0:
        raise _host_error(rc)
    bins = n * -(-h // bin_size.value) * -(-w // bin_size.value) if n else 0
    bin_start, bin_prims = np.zeros(bins + 1, np.int32), np.zeros(max(1, n_refs.value), np.int32)
    rc = lib().ck_overlay_plan(*args, bin_start.ctypes.data_as(C.c_void_p), bin_prims.ctypes.data_as(C.c_void_p), n_refs.value,
                               C.byref(n_refs))
    if rc != 0:
        raise _host_error(rc)
    return bin_size.value, bin_start, bin_prims[:n_refs.value]


def overlay_glyph(ch):
    """the seven row bytes of the overlay font's glyph of byte `ch`, top row first, bit 4 = leftmost column -> (7,) uint8;
    a byte outside 32 .. 126 gives the glyph of '?' (host only)"""
    rows = np.zeros(7, np.uint8)
    rc = lib().ck_overlay_glyph(int(ch), rows.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise _host_error(rc)
    return rows


def get_perspective_transform(src4, dst4):
    """K7, host only (board/boardfinder.py:43-45)."""
    src = np.ascontiguousarray(src4, np.float32).reshape(4, 2)
    dst = np.ascontiguousarray(dst4, np.float32).reshape(4, 2)
    M = np.zeros(9, np.float64)
    rc = lib().ck_get_perspective_transform(src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                            M.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise CkError("degenerate quadrilateral")
    return M.reshape(3, 3)


def update_grid(lines, box, slot):
    """update_grid (stone/stonesfinder.py:888-947), host only: lines as cv2.HoughLinesP returns them ((k, 1, 4) or (k, 4)),
    box = getrect of the zone, slot = the int16 pair of the intersection, updated in place"""
    seg = np.ascontiguousarray(np.asarray(lines).reshape(-1, 4), np.int32)
    b = np.ascontiguousarray(box, np.int32)
    out = np.ascontiguousarray(slot, np.int16).copy()
    rc = lib().ck_update_grid(seg.ctypes.data_as(C.c_void_p), len(seg), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ZeroDivisionError("float division by zero") if rc == 1 else CkError("ck_update_grid: error %d" % rc)
    slot[:] = out


def ordered_hull(points):
    """imgutil.get_ordered_hull: convex hull of integer (x, y) points, clockwise on screen, nearest to the origin
    first -> list of (x, y) tuples (host only)"""
    pts = np.ascontiguousarray(np.asarray(points).reshape(-1, 2), np.int32)
    out, n = np.zeros((max(1, len(pts)), 2), np.int32), C.c_int32(0)
    rc = lib().ck_ordered_hull(pts.ctypes.data_as(C.c_void_p), len(pts), out.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc != 0:
        raise CkError("ck_ordered_hull: error %d" % rc)
    return [(int(x), int(y)) for x, y in out[:n.value]]


def _gathered(recs, order):
    """the records a fold reads where they lie, frame f at recs[order[f]] (or recs[f]) -> the number of frames"""
    _check_array(recs, None, REC_DTYPE, "records")
    if order is None:
        return len(recs)
    _check_array(order, None, np.int32, "order")
    return len(order)


class BoardFoldCore:
    """ck_boardfold: the ordered half of the automatic board finder (host only, no GPU needed)."""

    def __init__(self):
        self._h = C.c_void_p()
        if lib().ck_boardfold_create(C.byref(self._h)) != 0:
            raise CkError("ck_boardfold_create failed")
        self._out = np.zeros(16, np.int32)          # found, update, n_centers, pad, centers[8], stats[2]
        self._io32, self._io64 = np.zeros(2, np.int32), np.zeros(3, np.int64)      # ck_boardfold_run: (k, hold), (counter, seen, looked)

    def __del__(self):
        try:
            if self._h:
                lib().ck_boardfold_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def reset(self):
        lib().ck_boardfold_reset(self._h)

    def step(self, h, w, status, lines, counter, cur_hull):
        """-> (found, update, centers [(x, y), ...], stats (clusters, intersections) or None)"""
        lines = np.ascontiguousarray(lines, np.float32).reshape(-1, 2)
        hull = None if cur_hull is None else np.ascontiguousarray(cur_hull, np.int32).reshape(8)
        o = self._out
        base = o.ctypes.data
        rc = lib().ck_boardfold_step(self._h, int(h), int(w), int(status), lines.ctypes.data_as(C.c_void_p), len(lines),
                                     int(counter), None if hull is None else hull.ctypes.data_as(C.c_void_p),
                                     C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 16), C.c_void_p(base + 8),
                                     C.c_void_p(base + 48))
        if rc == 4:
            raise IndexError("corner hull has fewer than 4 vertices")      # what the reference raises (bf_auto.py:206)
        if rc != 0:
            raise CkError("ck_boardfold_step: error %d" % rc)
        cen = [(int(o[4 + 2 * i]), int(o[5 + 2 * i])) for i in range(int(o[2]))]
        return bool(o[0]), bool(o[1]), cen, (None if o[12] < 0 else (int(o[12]), int(o[13])))


    def run(self, h, w, recs, k, counter, hold, seen, looked, cur_hull, order=None, hold_after_same_hit=-1):
        """ck_boardfold_run over the REC_DTYPE array `recs` (frame f at recs[order[f]], or recs[f]) from frame k ->
        (k, counter, hold, seen, looked, found, update, centers, stats): stops after the first frame that changes the corners
        (with hold_after_same_hit < 0: after every hit), or at the end of the batch"""
        n = _gathered(recs, order)
        hull = None if cur_hull is None else np.ascontiguousarray(cur_hull, np.int32).reshape(8)
        io32, io64 = self._io32, self._io64
        io32[:] = (k, hold)
        io64[:] = (counter, seen, looked)
        o = self._out
        base, b32, b64 = o.ctypes.data, io32.ctypes.data, io64.ctypes.data
        rc = lib().ck_boardfold_run(self._h, int(h), int(w), recs.ctypes.data_as(C.c_void_p),
                                    None if order is None else order.ctypes.data_as(C.c_void_p), n, C.c_void_p(b32),
                                    C.c_void_p(b64), C.c_void_p(b32 + 4), C.c_void_p(b64 + 8),
                                    None if hull is None else hull.ctypes.data_as(C.c_void_p), int(hold_after_same_hit),
                                    C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 16), C.c_void_p(base + 8),
                                    C.c_void_p(base + 48))
        state = (int(io32[0]), int(io64[0]), int(io32[1]), int(io64[1]), int(io64[2]))
        if rc == 4:
            err = IndexError("corner hull has fewer than 4 vertices")      # what the reference raises (bf_auto.py:206)
            err.fold_state = state
            raise err
        if rc != 0:
            raise CkError("ck_boardfold_run: error %d" % rc)
        cen = [(int(o[4 + 2 * i]), int(o[5 + 2 * i])) for i in range(int(o[2]))]
        return state + (bool(o[0]), bool(o[1]), cen, (None if o[12] < 0 else (int(o[12]), int(o[13]))))


class PolicyCore:
    """ck_policy: SfNeural's emission policy over ordered runs of frames (host only, no GPU needed)."""
    SUGGEST, BULK = 1, 2

    def __init__(self, bg_init_frames=50):
        self._h = C.c_void_p()
        if lib().ck_policy_create(int(bg_init_frames), C.byref(self._h)) != 0:
            raise CkError("ck_policy_create failed")
        self._io = np.zeros(4, np.int32)            # frame, phase, kind, n_moves
        self._moves = np.zeros((2 * 361, 3), np.int32)

    def __del__(self):
        try:
            if self._h:
                lib().ck_policy_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def run(self, first_counter, region_label, region_conf, fgcount, board_of, apply, records=None, order=None):
        """Ordered run over n frames.  `board_of()` -> uint8 (19,19) goban as the controller holds it now;
        `apply(kind, [(color, r, c), ...], frame_index)` executes a request; if it raises, the run stops there and
        the rest of that frame is never done -- what an exception out of SfNeural._find means in the reference.
        `records`: a C-contiguous REC_DTYPE array to read the classifier's answers from (region_label / region_conf are
        then ignored: ck_policy_run_records, no copy of the two strided fields), frame f at records[order[f]] when `order`
        (int32) is given"""
        if records is not None:
            n = _gathered(records, order)
        else:
            rl = np.ascontiguousarray(region_label, np.uint8).reshape(-1, 100)
            rc = np.ascontiguousarray(region_conf, np.float64).reshape(-1, 100)
            n = len(rl)
            if len(rc) != n:
                raise CkError("region_conf of %d frames for region_label of %d" % (len(rc), n))
        fg = None
        if fgcount is not None:
            fg = np.ascontiguousarray(fgcount, np.int32).reshape(n, 361)
        io, mv = self._io, self._moves
        io[:] = 0
        b = io.ctypes.data
        while True:
            board = np.ascontiguousarray(board_of(), np.uint8).reshape(361)
            tail = (None if fg is None else fg.ctypes.data_as(C.c_void_p), board.ctypes.data_as(C.c_void_p), C.c_void_p(b),
                    C.c_void_p(b + 4), C.c_void_p(b + 8), mv.ctypes.data_as(C.c_void_p), len(mv), C.c_void_p(b + 12))
            if records is not None:
                rcode = lib().ck_policy_run_records(self._h, n, int(first_counter), records.ctypes.data_as(C.c_void_p),
                                                    None if order is None else order.ctypes.data_as(C.c_void_p), *tail)
            else:
                rcode = lib().ck_policy_run(self._h, n, int(first_counter), rl.ctypes.data_as(C.c_void_p),
                                            rc.ctypes.data_as(C.c_void_p), *tail)
            if rcode != 0:
                raise CkError("ck_policy_run: error %d" % rcode)
            if io[2] == 0:
                return
            # a request made in the first half of frame k leaves (k, 1); a lookback request leaves (k + 1, 0)
            frame = int(io[0]) if io[1] == 1 else int(io[0]) - 1
            apply(int(io[2]), [(int(c), int(r), int(k)) for c, r, k in mv[:io[3]]], frame)

    def state(self):
        t, hc = np.zeros((19, 19), np.uint8), np.zeros((19, 19), np.uint8)
        he, cf, fl = np.zeros((19, 19), np.int32), np.zeros((19, 19), np.float64), np.zeros(2, np.int32)
        lib().ck_policy_get_state(self._h, *(a.ctypes.data_as(C.c_void_p) for a in (t, hc, he, cf, fl)))
        return dict(targets=t, heat_color=hc, heat_energy=he, heat_conf=cf, has_sampled=bool(fl[0]), recolour_seen=int(fl[1]))

    def set_targets(self, targets):
        t = np.ascontiguousarray(targets, np.uint8).reshape(19, 19)
        lib().ck_policy_set_state(self._h, t.ctypes.data_as(C.c_void_p), -1)

    def set_sampled(self, flag=True):
        lib().ck_policy_set_state(self._h, None, int(bool(flag)))

    def watch(self, r, c, color, confidence=0.0, stamp=0):
        """start (or with color 0: drop) the watch on a prediction, as a fresh HeatPoint would"""
        if lib().ck_policy_watch(self._h, int(r), int(c), int(color), confidence, int(stamp)) != 0:
            raise CkError("ck_policy_watch: bad arguments")


_default_ctx = {}


def get_context(device=0):
    """Process-wide default context per device (finders create their own)."""
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
