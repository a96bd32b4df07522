"""Vision configuration constants with the same names the reference keeps in
camkifu/config/cvconf.py (canonical_size, frame_period, unsynced, file_fps, bfinders, sfinders)."""
from . import golib_shim

canonical_size = 20 * golib_shim.gsize      # 380: side of the straightened goban image
frame_period = 0.2                          # min seconds between two iterations (live input)
unsynced = "unsynced"                       # marker returned by lock-step file readers
file_fps = 5                                # target read rate for video files
downsample = 0                              # levels of cv2.pyrDown every frame goes through before a finder sees it (0: none)

# (module, class) pairs resolved by VManagerBase._reflect; first importable entry is the default
bfinders = [
    ("camkifu_amd.board.bf_auto", "BoardFinderAuto"),
    ("None", "None"),
]
sfinders = [
    ("camkifu_amd.stone.sf_neural", "SfNeural"),
    ("camkifu_amd.stone.sf_contours", "SfContours"),
    ("camkifu_amd.stone.sf_meta", "SfMeta"),
    ("camkifu_amd.stone.sf_clustering", "SfClustering"),
    ("None", "None"),
]
snapshot_dir = "."                          # where VManagerBase.snapshot writes snapshot-N.npy (or .jpg) / game-N.sgf
png_inflate = "host"                        # ImageCapture, read_pngs: where PNG files are inflated ("device": a wave per file on the GPU, for batches)
png_runs = False                            # VManagerBase.snapshot_png: the PNG encoder's runs mode (flat areas as deflate matches)
bf_loc = None
sf_loc = None
annotate = False                            # VidProcessor._show draws the metadata lines on the image before it queues it
screenw, screenh = 1920, 1080               # what imgutil._factor fits an image into (the reference asks the window system)
