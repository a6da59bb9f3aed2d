#!/usr/bin/env python3
"""Ground-truth masks for the real-frame segmentation tests, extracted from the reference's data/ directory:

  gtmask/<dataset>/*.jpg   data/<dataset>/gtmask/ of the frames already under frames/<dataset>/ (autodriving, uav, uavnew2,
                           tabletennis: three frames each), copied byte for byte.  The JPEGs are single-channel;
                           cv2.imread gives three equal channels, and the tests expand them the same way.

Data only -- no reference source text.  Run in the build container:  python tests/golden/gen_gtmask_fixtures.py"""
import os
import shutil

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/data"
DATASETS = ["autodriving", "uav", "uavnew2", "tabletennis"]


def main():
    for name in DATASETS:
        dst = os.path.join(HERE, "gtmask", name)
        os.makedirs(dst, exist_ok=True)
        for f in sorted(os.listdir(os.path.join(HERE, "frames", name))):
            shutil.copyfile(os.path.join(REF, name, "gtmask", f), os.path.join(dst, f))
            os.chmod(os.path.join(dst, f), 0o644)
        print(name, sorted(os.listdir(dst)))


if __name__ == "__main__":
    main()
