#!/usr/bin/env python
"""Write the golden of the optimised-table tests: Pillow's bytes with optimize=True (libjpeg's optimize_coding) of every
case of tests/jpeg_enc_opt_cases.py, into tests/golden/jpeg_enc_opt_cases.npz.  The inputs are not stored: the tests
regenerate them from the seeds.  Needs Pillow; runs on the CPU.

Every golden is compared with the reference (tests/jpeg_enc_opt_ref.py) as it is written: a mismatch stops the run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_enc_opt_cases as cases  # noqa: E402


def main():
    arrays = {}
    for case in cases.all_cases():
        data = cases.pillow_encode(cases.case_image(case), case[4], case[3], case[5])
        if data != cases.ref_encode(case):
            sys.exit("the reference differs from Pillow on " + cases.name_of(case))
        arrays[cases.name_of(case)] = np.frombuffer(data, np.uint8)
    np.savez_compressed(cases.GOLDEN, **arrays)
    print("%s: %d cases, %d bytes" % (os.path.basename(cases.GOLDEN), len(arrays), os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
