"""Frame sources and the capture readers of the reference's vision manager.

The reference reads frames with cv2.VideoCapture (FFmpeg) and wraps it in CaptureReaderBase /
CaptureReader (core/vmanager.py:461-635): when the input is a file, frames are skipped so that
only `cvconf.file_fps` frames per second of video are analysed, and every active VidProcessor
receives the same sequence of frames (lock-step).  Video decoding itself is a third-party
library there and is not rebuilt here; the captures below quack like cv2.VideoCapture over
uncompressed containers and over the one compressed format that decodes exactly, frame by frame: baseline JPEG
(ck_jpeg_decode: Huffman decoding on the host, everything after it in one GPU kernel, bit for bit cv2.imread's numbers):

  Y4MCapture   .y4m (YUV4MPEG2, 4:2:0 planar): frames stay I420 on the host (1.5 B/px) and are
               converted to BGR on the GPU (ck_i420_to_bgr) -- read() for one frame,
               read_raw_batch() for the fast-file pipeline; with `levels` set, read() converts and
               downsamples in one kernel (ck_i420_to_bgr_pyr)
  ArrayCapture an (n, h, w, 3) uint8 array or .npy file of BGR frames (memory mapped)
  AviMjpegCapture  .avi holding Motion-JPEG: the file is memory mapped, the frames' JPEG bytes go to the decoder as they lie
  ImageCapture     a .jpg / .jpeg or .png still, served over and over (the reference's CaptureReaderImg)

cv2 property ids are kept so CaptureReaderBase.skip reads like the reference's.

CaptureReaderBase.downsample(ret, img) is the reference's extension point of the same name
(core/vmanager.py:484-498, 527-533): every frame passes through it before a finder sees it.  Its one
documented use, cv2.pyrDown(img), is what `cvconf.downsample = N` switches on here (N levels, on the GPU).
"""
import os
import struct
import threading
import time

import numpy as np

from .. import cvconf

CAP_PROP_POS_FRAMES = 1
CAP_PROP_POS_AVI_RATIO = 2
CAP_PROP_FRAME_WIDTH = 3
CAP_PROP_FRAME_HEIGHT = 4
CAP_PROP_FPS = 5
CAP_PROP_FRAME_COUNT = 7


class ArrayCapture:
    """Frame source over an (n, h, w, 3) uint8 array (or a path to one saved with np.save).
    read() hands each consumer a private copy, like CaptureReader.read_file does."""

    def __init__(self, frames, fps=30.0):
        if isinstance(frames, str):
            frames = np.load(frames, mmap_mode="r")
        self.frames = frames
        self.pos = 0
        self.fps = float(fps)

    def isOpened(self):
        return self.frames is not None

    def read(self, caller=None):
        if self.frames is None or self.pos >= len(self.frames):
            return False, None
        frame = np.array(self.frames[self.pos], copy=True)
        self.pos += 1
        return True, frame

    def get(self, prop):
        if prop == CAP_PROP_POS_FRAMES:
            return float(self.pos)
        if prop == CAP_PROP_FRAME_COUNT:
            return float(len(self.frames))
        if prop == CAP_PROP_FPS:
            return self.fps
        if prop == CAP_PROP_POS_AVI_RATIO:
            return self.progress()
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self.frames.shape[2])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self.frames.shape[1])
        return 0.0

    def set(self, prop, value):
        if prop == CAP_PROP_POS_FRAMES:
            self.pos = int(value)          # assumption: the FFmpeg backend truncates a fractional frame index
            return True
        if prop == CAP_PROP_POS_AVI_RATIO:
            self.seek(value)
            return True
        return False

    def progress(self):
        return self.pos / max(1, len(self.frames))

    def seek(self, ratio):
        self.pos = int(ratio * len(self.frames))

    def release(self):
        pass


class Y4MError(ValueError):
    pass


def write_y4m(path, frames_i420, h, w, fps=(30, 1)):
    """frames_i420: iterable of flat I420 frames (h*w*3/2 bytes each)."""
    with open(path, "wb") as f:
        f.write(("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg\n" % (w, h, fps[0], fps[1])).encode())
        for fr in frames_i420:
            buf = np.ascontiguousarray(fr, np.uint8).reshape(-1)
            if buf.size != h * w * 3 // 2:
                raise Y4MError("frame has %d bytes, expected %d" % (buf.size, h * w * 3 // 2))
            f.write(b"FRAME\n")
            f.write(buf.tobytes())


class Y4MCapture:
    """cv2.VideoCapture look-alike over a YUV4MPEG2 4:2:0 file.  The file is memory mapped; frames are
    handed out as I420 (read_raw / read_raw_batch, zero copy) or as BGR through `convert`, a callable
    (i420_flat, h, w) -> (h, w, 3) BGR -- by default the GPU conversion of a camkifu_amd Context.
    `levels` > 0: read() hands out frames pyrDown-ed that many times, `convert` being called with levels=... (the
    Context's fused conversion); get(CAP_PROP_FRAME_WIDTH / HEIGHT) keep reporting the file's size, as cv2 would."""

    def __init__(self, path, convert=None, levels=0):
        self.path = path
        self.convert = convert
        self.levels = int(levels)
        self.pos = 0
        self._mm = None
        self._offsets = []
        try:
            self._open(path)
        except (OSError, Y4MError) as exc:
            self.error = exc
            self._mm = None

    def _open(self, path):
        mm = np.memmap(path, dtype=np.uint8, mode="r")
        end = min(len(mm), 4096)
        head = bytes(mm[:end])
        nl = head.find(b"\n")
        if not head.startswith(b"YUV4MPEG2") or nl < 0:
            raise Y4MError("not a YUV4MPEG2 file: " + path)
        self.w = self.h = None
        self.fps = 30.0
        chroma = "420"
        for tok in head[:nl].split(b" ")[1:]:
            tag, val = tok[:1], tok[1:].decode()
            if tag == b"W":
                self.w = int(val)
            elif tag == b"H":
                self.h = int(val)
            elif tag == b"F":
                num, den = val.split(":")
                self.fps = float(num) / float(den) if float(den) else 30.0
            elif tag == b"C":
                chroma = val
        if not self.w or not self.h:
            raise Y4MError("missing W/H in the stream header")
        if not chroma.startswith("420") or "p1" in chroma:      # 420jpeg / 420mpeg2 / 420paldv; no high bit depth
            raise Y4MError("only 8-bit 4:2:0 is supported, got C" + chroma)
        if (self.w | self.h) & 1:
            raise Y4MError("odd dimensions are not supported")
        self.fsize = self.h * self.w * 3 // 2
        # frame index: every frame starts with a "FRAME[ params]\n" line
        off, offsets = nl + 1, []
        n = len(mm)
        while off + 6 <= n:
            line_end = off + 5
            if bytes(mm[off:off + 5]) != b"FRAME":
                raise Y4MError("corrupt frame header at byte %d" % off)
            while line_end < n and mm[line_end] != 0x0A:
                line_end += 1
            data = line_end + 1
            if data + self.fsize > n:
                break                                        # truncated last frame: ignored
            offsets.append(data)
            off = data + self.fsize
        self._mm, self._offsets = mm, offsets

    def isOpened(self):
        return self._mm is not None

    def __len__(self):
        return len(self._offsets)

    def read_raw(self):
        """next frame as a flat I420 view into the mapping (no copy), or None at the end"""
        if self._mm is None or self.pos >= len(self._offsets):
            return None
        o = self._offsets[self.pos]
        self.pos += 1
        return self._mm[o:o + self.fsize]

    def read_raw_batch(self, indices, out=None):
        """frames `indices` stacked into an (len, fsize) uint8 array (`out` may be a reusable, e.g.
        pinned, buffer).  Does not move the read position."""
        if out is None:
            out = np.empty((len(indices), self.fsize), np.uint8)
        for k, i in enumerate(indices):
            o = self._offsets[i]
            out[k] = self._mm[o:o + self.fsize]
        return out[:len(indices)]

    def read(self, caller=None):
        raw = self.read_raw()
        if raw is None:
            return False, None
        convert = self.convert
        if convert is None:
            from .. import capi
            convert = capi.get_context().i420_to_bgr
            self.convert = convert
        raw = np.ascontiguousarray(raw)
        if self.levels:
            return True, np.asarray(convert(raw, self.h, self.w, levels=self.levels))
        return True, np.asarray(convert(raw, self.h, self.w))

    def get(self, prop):
        if prop == CAP_PROP_POS_FRAMES:
            return float(self.pos)
        if prop == CAP_PROP_FRAME_COUNT:
            return float(len(self._offsets))
        if prop == CAP_PROP_FPS:
            return self.fps
        if prop == CAP_PROP_POS_AVI_RATIO:
            return self.pos / max(1, len(self._offsets))
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self.w)
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self.h)
        return 0.0

    def set(self, prop, value):
        if prop == CAP_PROP_POS_FRAMES:
            self.pos = int(value)
            return True
        if prop == CAP_PROP_POS_AVI_RATIO:
            self.pos = int(value * len(self._offsets))
            return True
        return False

    def progress(self):
        return self.pos / max(1, len(self._offsets))

    def seek(self, ratio):
        self.pos = int(ratio * len(self._offsets))

    def release(self):
        self._mm = None


class AviError(ValueError):
    pass


def write_mjpeg_avi(path, jpeg_frames, h, w, fps=(30, 1)):
    """a RIFF 'AVI ' container around JPEG byte strings (one '00dc' chunk each; an empty string gives the zero-length
    chunk that stands for "repeat the previous frame").  Container only: nothing is encoded here.  fps: (rate, scale)."""
    frames = [bytes(f) for f in jpeg_frames]
    rate, scale = (int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else (int(round(float(fps) * 1000)), 1000)

    def chunk(cc, body):
        return cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")

    def lst(kind, body):
        return b"LIST" + struct.pack("<I", len(body) + 4) + kind + body

    biggest = max([len(f) for f in frames] or [0])
    avih = struct.pack("<14I", int(1e6 * scale / max(1, rate)), 0, 0, 0, len(frames), 0, 1, biggest, w, h, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, scale, rate, 0, len(frames), biggest, 0xFFFFFFFF, 0,
                                          0, 0, w, h)
    strf = struct.pack("<IiiHH", 40, w, h, 1, 24) + b"MJPG" + struct.pack("<IiiII", w * h * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi = lst(b"movi", b"".join(chunk(b"00dc", f) for f in frames))
    body = b"AVI " + hdrl + movi
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


AVI_MAX_BYTES = 1 << 30          # what AviMjpegCapture reads of a file: the first RIFF chunk, no OpenDML extension


def _default_encode():
    from .. import capi
    return capi.get_context().jpeg_encode


def write_jpeg(path, bgr, quality=90, sampling=None, encode=None, restart_interval=0, optimize=False):
    """one BGR image (h, w, 3), a numpy array or a tensor in HBM, as a baseline JPEG still: the bytes libjpeg's default
    compressor writes (cv2.imwrite, PIL.Image.save).  sampling: capi.CK_JPEG_* (4:2:0 when None); encode: a callable
    (frames, quality=, sampling=) -> [bytes], by default jpeg_encode of the process-wide Context; restart_interval: MCUs
    between restart markers (0: none; handed to `encode` as restart_interval= only when set); optimize: Huffman tables
    fitted to the image, a smaller file of the same pixels (handed on as optimize=True only when set).  -> bytes written"""
    from .. import capi
    if len(bgr.shape) != 3 or bgr.shape[2] != 3:
        raise ValueError("write_jpeg takes one (h, w, 3) image, got %r" % (tuple(bgr.shape),))
    encode = encode or _default_encode()
    extra = dict(restart_interval=int(restart_interval)) if restart_interval else {}
    if optimize:
        extra["optimize"] = True
    data = encode(bgr[None], quality=quality, sampling=capi.CK_JPEG_420 if sampling is None else sampling, **extra)[0]
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def write_png(path, bgr, encode=None, filter=None, runs=None):
    """one BGR image (h, w, 3), a numpy array or a tensor in HBM, as a PNG still: 8-bit RGB, lossless, what any viewer and
    cv2.imread open.  encode: a callable (frames, filter=) -> [bytes], by default png_encode of the process-wide Context;
    filter: None chooses per row (libpng's heuristic), 0 .. 4 forces one type; runs: True / False asks the encoder for its
    runs mode (flat areas shrink as under zlib's Z_RLE) or its literal-only mode, None leaves it what the context has set --
    the keyword reaches `encode` only when it is not None.  -> bytes written"""
    if len(bgr.shape) != 3 or bgr.shape[2] != 3:
        raise ValueError("write_png takes one (h, w, 3) image, got %r" % (tuple(bgr.shape),))
    if encode is None:
        from .. import capi
        encode = capi.get_context().png_encode
    data = (encode(bgr[None], filter=filter) if runs is None else encode(bgr[None], filter=filter, runs=runs))[0]
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read_pngs(paths, to_device=None, inflate=None):
    """PNG stills -> their BGR images, in the order of `paths`: the files are grouped by (height, width) and every group is
    decoded in one png_decode of the process-wide Context -- the call in which the device inflate has a batch to work on.
    to_device: a torch device to leave the images in HBM; inflate: "host" / "device", None takes cvconf.png_inflate.
    -> a list of (h, w, 3) arrays (views into their group's batch).  OSError for a file that cannot be read, CkError for
    one the reader refuses: its `bad_frame` is the index into `paths`."""
    from .. import capi, cvconf
    ctx = capi.get_context()
    files = []
    for p in paths:
        with open(p, "rb") as f:
            files.append(f.read())
    groups = {}
    for k, data in enumerate(files):
        try:
            info = capi.png_header(data)
        except capi.CkError as e:
            e.bad_frame = k
            raise
        groups.setdefault((info["h"], info["w"]), []).append(k)
    images = [None] * len(files)
    for members in groups.values():
        try:
            batch = ctx.png_decode([files[k] for k in members], to_device=to_device, inflate=cvconf.png_inflate if inflate is None else inflate)
        except capi.CkError as e:
            if e.bad_frame is not None:
                e.bad_frame = members[e.bad_frame]
            raise
        for i, k in enumerate(members):
            images[k] = batch[i]
    return images


class MjpegWriter:
    """Motion-JPEG into a RIFF 'AVI ' file, streamed: write(frames) encodes a batch -- (n, h, w, 3) BGR, a numpy array or a
    tensor in HBM -- and appends one '00dc' chunk per frame; close() patches the RIFF, movi, avih and strh fields that depend
    on the frame count and appends the 'idx1' index.  The layout is write_mjpeg_avi's, so AviMjpegCapture reads it back.
    `encode`: a callable (frames, quality=, sampling=) -> [bytes], by default jpeg_encode of the process-wide Context.
    `restart_interval`: MCUs between restart markers (0: none; handed to `encode` as restart_interval= only when set) -- a
    film with them decodes in parallel pieces in the device entropy mode (Context.jpeg_set_entropy).
    `optimize`: Huffman tables fitted to every frame, a smaller film of the same pixels (handed on as optimize=True only when set).
    A batch that would take the file past AVI_MAX_BYTES raises AviError before any of it is written (the reader stops
    there: no OpenDML); the file can still be closed and holds the batches before.  Use as a context manager, or close()."""

    def __init__(self, path, h, w, fps=30.0, quality=90, sampling=None, encode=None, restart_interval=0, optimize=False):
        from .. import capi
        self.path, self.h, self.w = path, int(h), int(w)
        self.quality = int(quality)
        self.restart_interval = int(restart_interval)
        self.optimize = bool(optimize)
        self.sampling = capi.CK_JPEG_420 if sampling is None else int(sampling)
        self.encode = encode
        self.rate, self.scale = (int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else (int(round(float(fps) * 1000)), 1000)
        self.frames = 0
        self._index = []                     # (offset from the 'movi' tag, length) of every chunk
        self._biggest = 0
        head = self._headers(0)
        self._movi = len(head) - 4           # where the 'movi' tag stands
        self._end = len(head)                # where the next chunk goes
        self._f = open(path, "wb")
        self._f.write(head)

    def _headers(self, chunk_bytes):
        """everything up to the first chunk, for the frames written so far, whose chunks take chunk_bytes"""
        def chunk(cc, body):
            return cc + struct.pack("<I", len(body)) + body

        def lst(kind, body):
            return b"LIST" + struct.pack("<I", len(body) + 4) + kind + body

        w, h, n = self.w, self.h, self.frames
        avih = struct.pack("<14I", int(1e6 * self.scale / max(1, self.rate)), 0, 0, 0x10, n, 0, 1, self._biggest, w, h, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._biggest,
                                              0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH", 40, w, h, 1, 24) + b"MJPG" + struct.pack("<IiiII", w * h * 3, 0, 0, 0, 0)
        hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
        head = b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + chunk_bytes) + b"movi"
        return b"RIFF" + struct.pack("<I", len(head) + chunk_bytes + 8 + 16 * n) + head

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def write(self, frames):
        if self._f is None:
            raise AviError("the writer is closed")
        shp = tuple(frames.shape)
        if len(shp) == 3:
            frames, shp = frames[None], (1,) + shp
        if len(shp) != 4 or shp[1:] != (self.h, self.w, 3):
            raise ValueError("frames of %r where the file holds %dx%d BGR" % (shp, self.w, self.h))
        if shp[0] == 0:
            return 0
        if self.encode is None:
            self.encode = _default_encode()
        extra = dict(restart_interval=self.restart_interval) if self.restart_interval else {}
        if self.optimize:
            extra["optimize"] = True
        streams = self.encode(frames, quality=self.quality, sampling=self.sampling, **extra)
        if len(streams) != shp[0]:
            raise AviError("the encoder gave %d streams for %d frames" % (len(streams), shp[0]))
        sizes = [len(s) for s in streams]
        grown = self._end + sum(8 + n + (n & 1) for n in sizes)
        if grown + 8 + 16 * (self.frames + len(sizes)) > AVI_MAX_BYTES:
            raise AviError("%s would pass %d bytes with these %d frames: AVI files above 1 GiB (OpenDML) are not written"
                           % (self.path, AVI_MAX_BYTES, len(sizes)))
        for s, n in zip(streams, sizes):
            self._index.append((self._end - self._movi, n))
            self._f.write(b"00dc" + struct.pack("<I", n))
            self._f.write(s)
            if n & 1:
                self._f.write(b"\0")
            self._end += 8 + n + (n & 1)
        self.frames += len(sizes)
        self._biggest = max([self._biggest] + sizes)
        return len(sizes)

    def close(self):
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * self.frames)
                    + b"".join(b"00dc" + struct.pack("<III", 0x10, o, n) for o, n in self._index))
            f.seek(0)
            f.write(self._headers(self._end - self._movi - 4))
        finally:
            f.close()


class AviMjpegCapture:
    """cv2.VideoCapture look-alike over Motion-JPEG in an AVI container.  The file is memory mapped and walked once:
    hdrl/avih, the first 'vids' stream's strh (fps = dwRate / dwScale) and strf (biCompression or the stream handler must
    be MJPG), then the ##dc / ##db chunks of movi in file order; an idx1 chunk is ignored.  Frames are handed out as their
    JPEG bytes (read_raw_batch, views of the mapping) or as BGR through `decode`, a callable (list of byte strings) ->
    (n, h, w, 3) BGR -- by default jpeg_decode of the process-wide Context.

    An empty chunk, or one whose headers the decoder refuses (capi.jpeg_probe), stands for a repeat of the previous good
    frame, as players take it; such chunks are counted in `.damaged`.  Before any good frame it is a failed read.
    Only the first video stream is read: chunks of other streams (a second video stream, audio) are passed over.
    OpenDML ('AVIX') extensions are not read: frames beyond the first RIFF chunk (files above 1 GiB or so) are ignored."""

    def __init__(self, path, decode=None):
        self.path = path
        self.decode = decode
        self.pos = 0
        self.damaged = 0
        self.error = None
        self._mm = None
        self._chunks = []                       # (offset, length) of every video chunk
        self._good = None                       # per chunk: index of the chunk whose picture it shows (-1: none yet)
        try:
            self._open(path)
        except (OSError, AviError, struct.error) as exc:
            self.error = exc
            self._mm = None

    def _open(self, path):
        mm = np.memmap(path, dtype=np.uint8, mode="r")
        if len(mm) < 12 or bytes(mm[:4]) != b"RIFF" or bytes(mm[8:12]) != b"AVI ":
            raise AviError("not a RIFF AVI file: " + path)
        end = min(len(mm), 8 + struct.unpack("<I", bytes(mm[4:8]))[0])
        st = dict(w=0, h=0, fps=0.0, handler=b"", comp=b"", vids=False, done=False, streams=0, tag=b"")
        chunks = []
        # the RIFF tree, walked with a stack of our own (no recursion: a file decides how deep its lists nest).  An entry
        # is (next byte, end, inside movi); 'rec ' lists inside movi group chunks and are walked like movi itself.
        stack = [(12, end, False)]
        while stack:
            p, stop, in_movi = stack.pop()
            if p + 8 > stop:
                continue
            cc = bytes(mm[p:p + 4])
            ln = struct.unpack("<I", bytes(mm[p + 4:p + 8]))[0]
            body = p + 8
            stack.append((body + ln + (ln & 1), stop, in_movi))              # the sibling after this chunk
            if cc == b"LIST":
                if len(stack) > 64:
                    raise AviError("lists nested more than 64 deep")
                if body + 4 <= stop:
                    kind = bytes(mm[body:body + 4])
                    stack.append((body + 4, min(stop, body + ln), kind == b"movi" or (in_movi and kind == b"rec ")))
            elif cc == b"strh":
                hd = bytes(mm[body:min(stop, body + ln)])
                if not st["done"]:
                    st["vids"] = hd[:4] == b"vids"
                    if st["vids"] and len(hd) >= 28:
                        st["handler"] = hd[4:8]
                        scale, rate = struct.unpack("<II", hd[20:28])
                        st["fps"] = rate / scale if scale else 0.0
                        st["tag"] = b"%02d" % st["streams"]                # its chunks are '##dc' / '##db', ## its number
                st["streams"] += 1
            elif cc == b"strf" and st["vids"] and not st["done"]:
                bi = bytes(mm[body:min(stop, body + ln)])
                if len(bi) < 20:
                    raise AviError("short stream format")
                st["w"], st["h"] = struct.unpack("<ii", bi[4:12])
                st["h"] = abs(st["h"])
                st["comp"] = bi[16:20]
                st["done"] = True
            elif in_movi and st["done"] and cc[:2] == st["tag"] and cc[2:4] in (b"dc", b"db"):
                chunks.append((body, max(0, min(ln, stop - body))))
        if not st["done"]:
            raise AviError("no video stream")
        if b"MJPG" not in (st["comp"].upper(), st["handler"].upper()):
            raise AviError("the video stream is %r / %r, only MJPG is read" % (st["comp"], st["handler"]))
        if st["w"] <= 0 or st["h"] <= 0:
            raise AviError("bad frame size")
        self.w, self.h, self.fps = st["w"], st["h"], st["fps"] or 30.0
        # which picture every chunk shows: itself when its headers are a baseline JPEG of the stream's size, else the
        # last chunk that was
        from .. import capi
        good, last = [], -1
        for k, (o, ln) in enumerate(chunks):
            ok = False
            if ln:
                try:
                    info = capi.jpeg_probe(mm[o:o + ln])
                    ok = info["h"] == self.h and info["w"] == self.w
                except capi.CkError:
                    ok = False
            if ok:
                last = k
            else:
                self.damaged += 1
            good.append(last)
        self._mm, self._chunks, self._good = mm, chunks, good

    def isOpened(self):
        return self._mm is not None

    def __len__(self):
        return len(self._chunks)

    def read_raw_batch(self, indices):
        """the JPEG bytes of frames `indices` as views of the mapping (no copy); a repeat frame gives the bytes of the
        frame it repeats, None where there is no good frame yet.  Does not move the read position."""
        out = []
        for i in indices:
            g = self._good[i]
            out.append(None if g < 0 else self._mm[self._chunks[g][0]:self._chunks[g][0] + self._chunks[g][1]])
        return out

    def read(self, caller=None):
        if self._mm is None or self.pos >= len(self._chunks):
            return False, None
        raw = self.read_raw_batch([self.pos])[0]
        self.pos += 1
        if raw is None:
            return False, None
        decode = self.decode
        if decode is None:
            from .. import capi
            decode = capi.get_context().jpeg_decode
            self.decode = decode
        return True, np.asarray(decode([raw]))[0]

    def get(self, prop):
        if prop == CAP_PROP_POS_FRAMES:
            return float(self.pos)
        if prop == CAP_PROP_FRAME_COUNT:
            return float(len(self._chunks))
        if prop == CAP_PROP_FPS:
            return self.fps
        if prop == CAP_PROP_POS_AVI_RATIO:
            return self.progress()
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self.w)
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self.h)
        return 0.0

    def set(self, prop, value):
        if prop == CAP_PROP_POS_FRAMES:
            self.pos = int(value)
            return True
        if prop == CAP_PROP_POS_AVI_RATIO:
            self.seek(value)
            return True
        return False

    def progress(self):
        return self.pos / max(1, len(self._chunks))

    def seek(self, ratio):
        self.pos = int(ratio * len(self._chunks))

    def release(self):
        self._mm = None


class ImageCapture:
    """The reference's CaptureReaderImg (core/vmanager.py:638-660) for a .jpg / .jpeg or .png still: the image is decoded
    once (`decode` as for AviMjpegCapture; by default jpeg_decode or, for a file that starts with the PNG signature,
    png_decode of the process-wide Context) and every read() returns a copy of it; get() returns 0 whatever is asked, and
    nothing sleeps."""

    def __init__(self, path, decode=None):
        self.path = path
        self.img = None
        self.error = None
        try:
            with open(path, "rb") as f:
                data = f.read()
            if decode is None:
                from .. import capi
                ctx = capi.get_context()
                decode = ctx.jpeg_decode
                if data[:8] == PNG_SIGNATURE:
                    from .. import cvconf
                    decode = ctx.png_decode                  # (the keyword reaches it only when cvconf asks for the device inflate)
                    if cvconf.png_inflate != "host":
                        decode = lambda streams: ctx.png_decode(streams, inflate=cvconf.png_inflate)
            self.img = np.asarray(decode([data]))[0]
        except (OSError, RuntimeError) as exc:
            self.error = exc

    def isOpened(self):
        return self.img is not None

    def read(self, caller=None):
        if self.img is None:
            return False, None
        return True, self.img.copy()

    def get(self, prop):
        return 0

    def set(self, prop, value):            # (the reference's reader ignores every other call)
        return False

    def seek(self, ratio):
        pass

    def progress(self):
        return 0

    def release(self):
        pass


def open_capture(video, convert=None):
    """the capture for a controller's `video` attribute: an array, a .npy path, a .y4m path, an MJPEG .avi path or a
    .jpg / .jpeg / .png still"""
    if isinstance(video, str) and video.lower().endswith(".y4m"):
        return Y4MCapture(video, convert=convert)
    if isinstance(video, str) and video.lower().endswith(".avi"):
        return AviMjpegCapture(video)
    if isinstance(video, str) and video.lower().endswith((".jpg", ".jpeg", ".png")):
        return ImageCapture(video)
    return ArrayCapture(video)


def file_frame_indices(nframes, fps, rate=None, start=0):
    """the frame numbers CaptureReaderBase.skip() makes a file reader visit (core/vmanager.py:511-525):
    before EVERY read the position advances by max(1, fps / rate) and the read itself advances by one,
    so the period is fps/rate + 1 and the first frame analysed is not frame 0."""
    rate = cvconf.file_fps if rate is None else rate
    out, idx = [], float(start)
    while True:
        idx += max(1, fps / rate)
        idx = min(idx, nframes)
        if int(idx) >= nframes:
            return out
        out.append(int(idx))
        idx = int(idx) + 1.0


class CaptureReaderBase:
    """What a manager puts between its finders and the capture: `read(caller)` is taken over, every other
    attribute is the capture's.  A video FILE is thinned to `fps` analysed frames per second of footage with
    the reference's arithmetic (core/vmanager.py:510-525; see file_frame_indices); other sources pass through.
    Every frame read goes through `downsample(ret, img)` before it is handed out.
    `ctx`: the Context that downsamples (default: the process-wide one)."""

    def __init__(self, capture, vmanager, fps=None, ctx=None):
        self.__dict__.update(capture=capture, vmanager=vmanager,
                             frame_rate=cvconf.file_fps if fps is None else fps, ctx=ctx)

    def __getattr__(self, attr):                       # only reached for names this object does not define
        return getattr(self.__dict__["capture"], attr)

    def is_file(self):
        video = getattr(getattr(self.vmanager, "controller", None), "video", None)
        return isinstance(video, str) and os.path.isfile(video)

    def advance(self):
        """move the read position forward by the thinning stride (never beyond the last frame)"""
        cap = self.capture
        target = cap.get(CAP_PROP_POS_FRAMES) + max(1, cap.get(CAP_PROP_FPS) / self.frame_rate)
        cap.set(CAP_PROP_POS_FRAMES, min(target, cap.get(CAP_PROP_FRAME_COUNT)))

    skip = advance

    def read_capture(self):
        """capture.read() through the downsample hook.  A capture that downsamples while it converts (Y4MCapture's
        `levels`) is told the configured level first, and the hook then leaves its frames alone."""
        cap = self.capture
        if hasattr(cap, "levels"):
            cap.levels = int(cvconf.downsample or 0)
        return self.downsample(*cap.read())

    def downsample(self, ret, img):
        """The reference's extension point (core/vmanager.py:527-533), with its one documented use built in:
        `cvconf.downsample` = N > 0 hands every good frame out as N levels of cv2.pyrDown (ctx.pyr_down); 0 is the
        identity.  A failed read and the `unsynced` marker pass through untouched.  A subclass may override it (and then
        leaves cvconf.downsample at 0)."""
        levels = int(cvconf.downsample or 0)
        if not levels or not ret or img is None or isinstance(img, str):
            return ret, img
        if getattr(self.capture, "levels", 0) == levels:
            return ret, img                            # the capture has downsampled already
        ctx = self.ctx
        if ctx is None:
            from .. import capi
            ctx = capi.get_context()
        return ret, np.asarray(ctx.pyr_down(img, levels))

    def read(self, caller=None):
        if self.is_file():
            self.advance()
        return self.read_capture()


class CaptureReader(CaptureReaderBase):
    """Lock-step serving for the threaded manager (what core/vmanager.py:528-635 is for): every finder that is
    currently able to read gets frame k before anybody gets frame k+1.

    Built as a generation counter under one condition variable: the reader holds (generation, frame); a
    consumer remembers the last generation it took and sleeps on the condition while that is still the current
    one; whoever completes the set of consumers for a generation fetches the next frame and wakes the others.
    A consumer therefore sees every frame exactly once -- the reference's reader lets the thread served last
    walk away with the following frame (and sometimes see it twice), a timing artefact that is not mirrored."""

    def __init__(self, capture, vmanager, fps=None, ctx=None):
        super().__init__(capture, vmanager, fps, ctx)
        self.__dict__.update(_cv=threading.Condition(), _gen=0, _frame=None, _taken={}, unsync=False,
                             sleep_time=0.05)

    def _consumers(self):
        ready = []
        for thread in getattr(self.vmanager, "processes", ()):
            try:
                if thread.ready_to_read():
                    ready.append(thread.processor)
            except AttributeError:
                continue
        return ready

    def _fetch(self, first):
        """under the lock: load the next generation (downsampled once, whatever the number of consumers)"""
        if not first:
            self.advance()
        self._frame = self.read_capture()
        self._gen += 1
        if not first:
            self.vmanager.vid_progress(self.capture.get(CAP_PROP_POS_AVI_RATIO) * 100)
        self._cv.notify_all()

    def _maybe_turn_over(self):
        if all(self._taken.get(c) == self._gen for c in self._consumers()):
            self._fetch(first=False)

    def read(self, caller=None):
        if not self.is_file():
            return self.read_capture()
        with self._cv:
            if self._gen == 0:
                self._fetch(first=True)
            while not self.unsync and self._taken.get(caller) == self._gen:
                self._cv.wait(self.sleep_time)
                self._maybe_turn_over()                # a finder may have stopped being ready meanwhile
            if self.unsync:
                return False, cvconf.unsynced
            ok, img = self._frame
            self._taken[caller] = self._gen
            self._maybe_turn_over()
        return (ok, img.copy()) if ok else (ok, img)   # consumers may write on their image

    def unsync_threads(self, unsync):
        """True: wake everybody up with the `unsynced` marker (the manager is stopping its finders)"""
        with self._cv:
            self.unsync = bool(unsync)
            self._cv.notify_all()
