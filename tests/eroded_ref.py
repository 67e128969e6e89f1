"""Test-side restatement of the reference's PostProcInstErodedMap (loader/postproc.py:147-265, the IP-ERODED-3 / -11 codes), composed from the
oracle's primitives (oracle/postproc_ref.py: label4, dilate_ellipse, fill_holes -- each pinned to scipy / the documented OpenCV span formula
by its own tests) and numpy.  tests/tools/gen_golden_eroded.py asserts that it equals the reference's own class on every case of
tests/golden/pp_eroded.npz before it writes the fixture; the GPU tests use it where no stored map exists (the 2048^2 nuclei map, the tile
driver's own canvases)."""
import numpy as np

from oracle import postproc_ref as pr

MIN_SIZE = {"GLAND": 1500, "LUMEN": 150, "NUCLEI": 8}  # morphology.remove_small_objects(min_size=...)   (:156, :188, :220)
KSIZE = {"GLAND": 11, "LUMEN": 3, "NUCLEI": 3}         # cv2.getStructuringElement(MORPH_ELLIPSE, (ksize, ksize))   (:151, :183, :215)


def proc(inner, tissue):
    """inner: (H,W) or (H,W,1) float map -> float64 (H,W) instance map, as the reference's __proc_gland / __proc_lumen / __proc_nuclei return it."""
    t = tissue.upper()
    a = np.asarray(inner, dtype=np.float32)
    if a.ndim == 3:
        assert a.shape[2] == 1
        a = a[..., 0]
    H, W = a.shape
    fg = a > 0.5
    lab, n = pr.label4(fg)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= MIN_SIZE[t]  # remove_small_objects drops components SMALLER than min_size
    keep[0] = False
    lab, n = pr.label4(keep[lab])  # measurements.label of the filtered mask: ids in raster order of the first pixel
    out = np.zeros((H, W), np.float64)
    if n == 0 or lab.all():
        # id_list = np.unique(inst_lab).tolist()[1:] drops the SMALLEST label, which is meant to be the background: a map without a single background
        # pixel (one component, id 1) comes back empty
        return out
    k, pad = KSIZE[t], 2 * KSIZE[t]
    flat = np.flatnonzero(lab)
    ids = lab.ravel()[flat]
    ys, xs = np.divmod(flat, W)
    y_lo = np.full(n + 1, H, np.int64)
    x_lo = np.full(n + 1, W, np.int64)
    y_hi = np.zeros(n + 1, np.int64)
    x_hi = np.zeros(n + 1, np.int64)
    np.minimum.at(y_lo, ids, ys)
    np.minimum.at(x_lo, ids, xs)
    np.maximum.at(y_hi, ids, ys + 1)  # get_bounding_box (misc/utils.py:82-91): rmax / cmax are one past the last row / column
    np.maximum.at(x_hi, ids, xs + 1)
    for i in range(1, n + 1):
        y1, y2, x1, x2 = int(y_lo[i]), int(y_hi[i]), int(x_lo[i]), int(x_hi[i])
        y1 = y1 - pad if y1 - pad >= 0 else y1
        x1 = x1 - pad if x1 - pad >= 0 else x1
        x2 = x2 + pad if x2 + pad <= W - 1 else x2
        y2 = y2 + pad if y2 + pad <= H - 1 else y2
        crop = (lab[y1:y2, x1:x2] == i).astype(np.uint8)
        crop = pr.fill_holes(pr.dilate_ellipse(crop, k))
        out[y1:y2, x1:x2][crop > 0] = i
    return out


def cases(gold):
    """(name, tissue, float32 input map (H,W), expected int32 label map) of every case in pp_eroded.npz"""
    for name in [str(x) for x in gold["names"]]:
        yield name, str(gold["tissue/" + name]), gold["in/" + name].astype(np.float32), gold["out/" + name]
