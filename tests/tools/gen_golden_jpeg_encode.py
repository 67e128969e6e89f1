"""Writes tests/golden/jpeg_encode.npz: a few of the pictures of tests/jpeg_enc_ref.py with the quantised coefficients and tables THIS machine's PIL /
libjpeg wrote for them (read back through the entropy decoder, cerb_jpeg_decode_stream).  The encoder tests compare the numpy restatement with the live
PIL AND with these stored coefficients: a libjpeg build that encodes differently then shows up as a named difference
(test_this_pil_writes_the_fixture_coefficients), not as an encoder bug.

    python tests/tools/gen_golden_jpeg_encode.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import jpeg_enc_ref as er  # noqa: E402

NAMES = ["17x9_ss0_q75", "17x9_ss2_q30", "37x53_ss0_q95", "37x53_ss2_q75", "64x200_ss2_q100", "8x520_ss2_q75", "checker8_q100_ss2", "ff_bytes_ss0"]


def main():
    import PIL

    from cerberus_amd import jpeg_device as jd

    out = {"pil_version": np.array(PIL.__version__), "names": np.array(NAMES)}
    cases = {c[0]: c for c in er.cases()}
    for name in NAMES:
        _, img, q, ss = cases[name]
        rc, hdr, co = jd.decode_stream(er.pil_encode(img, q, ss))
        assert rc == jd.OK
        out["picture_" + name] = img
        out["quality_" + name] = np.array(q)
        out["subsampling_" + name] = np.array(ss)
        out["coefs_" + name] = co
        out["qluma_" + name] = np.array(hdr.q[0][:], np.uint16)
        out["qchroma_" + name] = np.array(hdr.q[1][:], np.uint16)
    path = os.path.join(os.path.dirname(HERE), "golden", "jpeg_encode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(NAMES), "pictures")


if __name__ == "__main__":
    main()
