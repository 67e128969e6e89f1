"""Writes tests/golden/jpeg_tiles.npz: the small seeded JPEG streams of tests/jpeg_ref.py and the pixels THIS machine's PIL / libjpeg returns for them.
The JPEG tests compare the native decoder with the live PIL AND with these stored pixels: a libjpeg build that decodes differently then shows up as a
named difference (test_this_pil_returns_the_fixture_pixels), not as a decoder bug.

    python tests/tools/gen_golden_jpeg.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jpeg_ref  # noqa: E402


def main():
    import PIL

    out = {"pil_version": np.array(PIL.__version__)}
    names = []
    for name, data, tabs, ph in jpeg_ref.cases():
        if name.startswith("240x240"):  # (the large size stays out of the repository: it is checked against the live PIL only)
            continue
        names.append(name)
        out["stream_" + name] = np.frombuffer(data, np.uint8)
        out["tables_" + name] = np.frombuffer(tabs or b"", np.uint8)
        out["photometric_" + name] = np.array(ph)
        out["pixels_" + name] = jpeg_ref.pil_pixels(data, tabs, ph)
    out["names"] = np.array(names)
    path = os.path.join(os.path.dirname(HERE), "golden", "jpeg_tiles.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "streams")


if __name__ == "__main__":
    main()
