#!/usr/bin/env python
"""Write the goldens of the JPEG encoder tests: Pillow's bytes (libjpeg's default compressor) of every case of
tests/jpeg_enc_cases.py, into tests/golden/jpeg_enc_cases.npz (the single cases) and jpeg_enc_cases_1.npz (the batch).
The inputs are not stored: the tests regenerate them from the seeds.  Needs Pillow; runs on the CPU.

Every golden is compared with the reference (tests/jpeg_enc_ref.py) as it is written: a mismatch stops the run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_enc_cases as cases  # noqa: E402


def main():
    single = {}
    for case in cases.all_cases():
        rows = 1 if case in cases.ROW_RESTART else 0
        data = cases.pillow_encode(cases.case_image(case), case[4], case[3], case[5], rows)
        if data != cases.ref_encode(case)[0]:
            sys.exit("the reference differs from Pillow on " + cases.name_of(case))
        single[cases.name_of(case)] = np.frombuffer(data, np.uint8)
    batch = {}
    for seed, case in enumerate(cases.BATCH):
        data = cases.pillow_encode(cases.case_image(case, seed), case[4], case[3], case[5])
        if data != cases.ref_encode(case, seed)[0]:
            sys.exit("the reference differs from Pillow on the batch frame %d" % seed)
        batch["%s_s%d" % (cases.name_of(case), seed)] = np.frombuffer(data, np.uint8)
    for name, arrays in (("jpeg_enc_cases.npz", single), ("jpeg_enc_cases_1.npz", batch)):
        path = os.path.join(cases.GOLDEN, name)
        np.savez_compressed(path, **arrays)
        print("%s: %d cases, %d bytes" % (name, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    main()
