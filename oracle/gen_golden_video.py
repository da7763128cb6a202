#!/usr/bin/env python
"""Generate ``tests/golden/video_iterators.npz``: what the REFERENCE's unmodified ``demos/video_iterator.py`` yields on
the decoder stand-ins of tests/test_video_results.py (its top-level ``import decord / cv2 / ffmpeg`` resolve to them).

Per case — rotation tag 0 / 90 / 180 / 270 (the 180 clip's read fails at frame 4), reader ``decord`` / ``cv2``, all frames
or ``frame_idxs=[4, 0, 3]`` — the iterator's ``len``, the frame ids it yields and the frames, stacked.  The clips
themselves are rebuilt from their seeds by the test, so only outputs are stored.

Runs only where the reference checkout is (SIAMMOT_REFERENCE, as oracle/gen_golden.py).
Usage:  python oracle/gen_golden_video.py
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import test_video_results as tv       # noqa: E402  (the stand-ins and clip cases the test replays)
from gen_golden import REFERENCE      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "video_iterators.npz")


def main():
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        tv._install_fake_decoders(mp)
        spec = importlib.util.spec_from_file_location("ref_video_iterator",
                                                      os.path.join(REFERENCE, "demos", "video_iterator.py"))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
        for case in tv.REFERENCE_ITERATOR_CASES:
            path, idxs, kind, key = tv._reference_iterator_case(case)
            it = ref.build_video_iterator(path, video_decode=kind)
            if idxs is not None:
                it = type(it)(path, frame_idxs=idxs)
            got = list(it())
            out[key + "/len"] = np.int64(len(it))
            out[key + "/ids"] = np.array([int(i) for i, _ in got], dtype=np.int64)
            out[key + "/frames"] = np.stack([f for _, f in got]).astype(np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d cases)" % (OUT, len(tv.REFERENCE_ITERATOR_CASES)))


if __name__ == "__main__":
    main()
