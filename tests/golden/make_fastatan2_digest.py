"""Records tests/golden/fastatan2_x1_digest.json: the digest of cv::fastAtan2(y, 1) of OpenCV 2.4.5 over all 2^32 float
bit patterns y (definition in tests/cv_pin.py), and its mismatches against the oracle's pmo_fast_atan2(y, 1).
sdm_selftest(10) must reproduce the digest from K1's fast_atan2_deg_x1 (tests/test_gpu_opencv_pin.py).
Needs the staged oracle/_ref/ (python __graft_entry__.py).  Run: python tests/golden/make_fastatan2_digest.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]
import cv_pin  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as d:
        bad, dig = cv_pin.Harness(d).all_patterns()
    doc = {"what": "sum mod 2^64 over all 2^32 float bit patterns i of mix64(i << 32 | bits(cvFastArctan(y_i, 1))), "
                   "NaN results as 0x7fc00000 (tests/cv_pin.py); OpenCV 2.4.5 as staged from the reference tree",
           "opencv": "2.4.5", "patterns": 2 ** 32, "digest": "0x%016x" % dig, "oracle_mismatches": bad}
    with open(os.path.join(HERE, "fastatan2_x1_digest.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(doc)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
